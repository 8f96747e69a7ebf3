"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on identical seeded inputs.

Bars: kNN indices bit-exact; EdgeConv features |d| <= 1e-5 + 1e-5*|ref| (the fused path
reassociates W.[x_i||x_j-x_i] into (W1-W2).x_i + W2.x_j); MET sums relative 1e-5 of sum|w*p|.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT_RTOL, FEAT_ATOL = 1e-5, 1e-5


def _default_path_only(switch, value, why):
    """tools/toggle_sweep.sh runs this suite under every diagnostic switch.  A test that asserts a property OF THE DEFAULT
    PATH ITSELF (its counters, its table layouts) has nothing to say under a switch that leaves that path; it says so here,
    with the reason, instead of failing."""
    import os
    if os.environ.get(switch) == value:
        pytest.skip(f"{switch}={value}: {why}")


def _ragged(sizes, D, seed, dup=False):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    x = torch.randn(N, D, generator=g)
    if dup:  # exact ties: duplicated rows and a lattice block
        x[N // 3] = x[1]
        x[N // 2] = x[1]
        x[-(N // 4):] = torch.round(x[-(N // 4):])
    counts = torch.tensor(sizes)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return x, batch, ptr


@pytest.mark.parametrize("sizes,D,k", [
    ([256], 32, 8),                       # BASELINE config 1 shape
    ([50, 450, 800], 32, 16),             # ragged (config 5 scaled down)
    ([1, 3, 0, 17, 129, 64, 2], 32, 16),  # n < k, single node, EMPTY event
    ([300, 200], 2, 20),                  # (eta,phi)-like 2-D space, reference's k=20
    ([130, 131], 5, 3),                   # odd D (padded path), small k
    ([400], 64, 33),                      # D=64 (DRN width), k -> 64-wide list
    ([700, 10], 16, 64),                  # maximum k
    ([900, 300, 21], 32, 20),             # the reference's k=20 (graph_met_network.py:63) on the matrix-core path
    ([500, 64], 32, 17),                  # 16 < k <= 20: same path, odd k
    ([600], 32, 24),                      # k > 20 at D = 32: exact kernel
])
def test_knn_bit_exact(dev, sizes, D, k):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    x, batch, ptr = _ragged(sizes, D, seed=100 + D + k, dup=True)
    nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
    t = dm.knn_table(x.to(dev), k, batch.to(dev), loop=True, num_events=len(sizes))
    assert torch.equal(t.nbr.cpu(), nbr_ref)
    assert torch.equal(t.dist.cpu(), dist_ref)  # distances are the same fmaf chain: bit-exact too
    from deepmetv2_amd import _native
    assert (t.nbr_local is not None) == (k in _native.LDS_GATHER_K)
    n2, d2, _ = _knn_with_stats(x.to(dev), ptr.to(dev), k)     # also checks the uint16 local table (any k)
    assert torch.equal(n2, nbr_ref) and torch.equal(d2, dist_ref)


@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_knn_graph_edge_index(dev, loop, flow):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    x, batch, ptr = _ragged([40, 3, 90], 8, seed=5, dup=True)
    ref = ref_ops.knn_graph(x, 6, batch, loop=loop, flow=flow)
    got = dm.knn_graph(x.to(dev), 6, batch.to(dev), loop=loop, flow=flow)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref)


def test_knn_full_size_event_property(dev):
    """BASELINE config-2 event size (4500 nodes, k=16): full oracle on one event + structural properties."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    x, batch, ptr = _ragged([4500, 4500], 32, seed=77)
    t = dm.knn_table(x.to(dev), 16, batch.to(dev), loop=True, num_events=2)
    nbr, dist = t.nbr.cpu(), t.dist.cpu()
    ref, _ = ref_ops.knn_table(x[:4500], torch.tensor([0, 4500]), 16)
    assert torch.equal(nbr[:4500], ref)
    assert torch.equal(nbr[:, 0], torch.arange(9000, dtype=torch.int32))      # self first (d = 0)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())                           # sorted
    assert bool(((nbr >= 4500) == (torch.arange(9000).view(-1, 1) >= 4500)).all())  # never crosses events


def test_knn_ragged_config5_full_size(dev):
    """BASELINE configs[4]: 64 events of 500..8000 nodes, k=16.  Full oracle on the smallest and the largest event,
    structural properties (self first, sorted, never crosses events) on all 270k nodes."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from oracle import ref_ops
    sizes = synth.ragged_sizes(64, 500, 8000, seed=99)
    x, batch, ptr = _ragged(sizes, 32, seed=55)
    N = x.shape[0]
    t = dm.knn_table(x.to(dev), 16, batch.to(dev), loop=True, num_events=64)
    nbr, dist = t.nbr.cpu(), t.dist.cpu()
    assert torch.equal(nbr[:, 0], torch.arange(N, dtype=torch.int32))
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    lo, hi = ptr[batch].view(-1, 1), ptr[batch + 1].view(-1, 1)
    assert bool(((nbr >= lo) & (nbr < hi)).all())
    for b in (int(torch.tensor(sizes).argmin()), int(torch.tensor(sizes).argmax())):
        s, e = int(ptr[b]), int(ptr[b + 1])
        ref, dref = ref_ops.knn_table(x[s:e], torch.tensor([0, e - s]), 16)
        assert torch.equal(nbr[s:e], ref + s) and torch.equal(dist[s:e], dref)


def _check_local_table(nbr, loc, ptr):
    """The uint16 event-local copy of the table (dmet_knn_local_f32) must describe the same graph; rows of events
    with more than 65535 nodes are unspecified."""
    nbr, loc, ptr = nbr.cpu(), loc.cpu(), ptr.cpu()
    counts = ptr[1:] - ptr[:-1]
    lo = torch.repeat_interleave(ptr[:-1], counts).to(torch.int32).view(-1, 1)
    rows = torch.repeat_interleave(counts <= 65535, counts)
    u = loc.to(torch.int32) & 0xFFFF
    back = torch.where(u == 0xFFFF, torch.full_like(u, -1), u + lo)
    assert torch.equal(back[rows], nbr[rows])


def _knn_with_stats(x, ptr, k):
    """Every call goes through dmet_knn_local_f32, so each writer of the table (in-place re-rank, tail re-rank,
    per-query fallback, exact tile kernel, merge) is also checked for the uint16 copy."""
    from deepmetv2_amd import _native
    st = {}
    nbr, dist, loc = _native.knn_local(x, ptr, k, stats=st)
    _check_local_table(nbr, loc, ptr)
    return nbr.cpu(), dist.cpu(), st


@pytest.mark.parametrize("case", ["gaussian", "outliers", "clusters", "identical", "lattice", "tiny_events"])
def test_knn_matrix_core_path_certification(dev, case):
    """K1, D = 32: the matrix-core filter + exact re-rank must return the oracle's bits on benign data WITHOUT falling
    back (flagged_tiles == 0), and on adversarial data (mass ties) through the certified fallback."""
    from oracle import ref_ops
    g = torch.Generator().manual_seed(7)
    k = 16
    if case == "tiny_events":
        sizes = [int(v) for v in torch.randint(0, 9, (700,), generator=g)]       # many events smaller than k, some empty
    else:
        sizes = [900, 37, 1500]
    N = sum(sizes)
    x = torch.randn(N, 32, generator=g)
    if case == "outliers":
        x[::97] *= 300.0                              # huge norms elsewhere in the event must not loosen the bound
    elif case == "clusters":
        centers = torch.randn(12, 32, generator=g) * 4
        x = centers[torch.randint(0, 12, (N,), generator=g)] + 1e-3 * torch.randn(N, 32, generator=g)
    elif case == "identical":
        x = torch.ones(N, 32) * 0.37                  # every distance ties: nothing can be certified
    elif case == "lattice":
        x = torch.round(x)                            # integer coordinates: many exact ties at the k-th distance
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)])
    nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
    nbr, dist, st = _knn_with_stats(x.to(dev), ptr.to(dev), k)
    assert torch.equal(nbr, nbr_ref) and torch.equal(dist, dist_ref)
    if case == "gaussian":
        assert st["flagged_queries"] == 0, st
    if case == "outliers":    # only the outlier queries themselves (1 in 97) may be beyond bf16-split certification
        assert st["flagged_queries"] <= N // 97 + 1, st
    if case == "identical" and os.environ.get("DMET_KNN_PATH") != "exact":
        assert st["flagged_tiles"] > 0, st            # the fallback really ran (under DMET_KNN_PATH=exact nothing is flagged:
                                                      # the exact kernel computes every tile by itself)


def test_knn_matrix_core_vs_exact_kernel_full_size(dev, monkeypatch):
    """BASELINE configs[1] shape (64 x 4500 x 32, k = 16): filter path == oracle on two events and structurally sound
    on all; flagged tiles stay rare on generic data."""
    from oracle import ref_ops
    g = torch.Generator().manual_seed(123)
    B, n, k = 64, 4500, 16
    x = torch.randn(B * n, 32, generator=g)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64)
    nbr, dist, st = _knn_with_stats(x.to(dev), ptr.to(dev), k)
    assert st["flagged_tiles"] <= 8, st
    for b in (0, 63):
        ref, dref = ref_ops.knn_table(x[b * n:(b + 1) * n], torch.tensor([0, n]), k)
        assert torch.equal(nbr[b * n:(b + 1) * n], ref + b * n) and torch.equal(dist[b * n:(b + 1) * n], dref)
    assert torch.equal(nbr[:, 0], torch.arange(B * n, dtype=torch.int32))
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    ev = torch.arange(B * n).view(-1, 1) // n
    assert bool(((nbr // n) == ev).all())


def test_knn_oversized_event_goes_to_exact_kernel(dev, monkeypatch):
    """An event of more than 65535 nodes does not fit the filter's 16-bit candidate ids: every query of it must be
    handed to the exact kernel (and a normal event next to it still takes the matrix-core path).  Reference: the
    exact kernel alone (DMET_KNN_PATH=exact; itself pinned to the oracle by test_knn_bit_exact), oracle on the small
    event."""
    from oracle import ref_ops
    g = torch.Generator().manual_seed(5)
    sizes = [66000, 700]
    x = torch.randn(sum(sizes), 32, generator=g)
    ptr = torch.tensor([0, 66000, 66700])
    nbr, dist, st = _knn_with_stats(x.to(dev), ptr.to(dev), 16)
    if os.environ.get("DMET_KNN_PATH") != "exact":      # (the property of the matrix-core path: the oversized event is handed over)
        assert st["flagged_queries"] >= 66000 and st["flagged_queries"] < 66000 + 16, st
    monkeypatch.setenv("DMET_KNN_PATH", "exact")
    nbr_x, dist_x, st_x = _knn_with_stats(x.to(dev), ptr.to(dev), 16)
    assert st_x["flagged_queries"] == 0
    assert torch.equal(nbr, nbr_x) and torch.equal(dist, dist_x)
    ref, dref = ref_ops.knn_table(x[66000:], torch.tensor([0, 700]), 16)
    assert torch.equal(nbr[66000:], ref + 66000) and torch.equal(dist[66000:], dref)


def test_knn_paths_agree_fuzz(dev, monkeypatch):
    """K1: 12 seeded random batches (ragged, tiny and empty events, k in {1, 8, 13, 16, 20}; gaussian, clustered with
    exact duplicates, heavy-tailed, rank-2 data): the matrix-core path (filter + certified re-rank + fallbacks) must
    return the exact kernel's bits everywhere (the exact kernel is pinned to the oracle by test_knn_bit_exact)."""
    g = torch.Generator().manual_seed(99)
    for it in range(12):
        B = int(torch.randint(1, 24, (1,), generator=g))
        hi = [1500, 120, 2500, 40, 700][it % 5]
        sizes = [int(v) for v in torch.randint(0, hi, (B,), generator=g)]
        N = sum(sizes)
        if N == 0:
            continue
        k = [16, 8, 20, 13, 1][it % 5]
        x = torch.randn(N, 32, generator=g)
        mode = it % 4
        if mode == 1:
            c = torch.randn(7, 32, generator=g) * 3
            x = c[torch.randint(0, 7, (N,), generator=g)] + 1e-2 * torch.randn(N, 32, generator=g)
            x[N // 2:N // 2 + N // 10] = x[:N // 10]
        elif mode == 2:
            x = x * torch.exp(2.0 * torch.randn(N, 1, generator=g))
        elif mode == 3:
            x = torch.randn(N, 2, generator=g) @ torch.randn(2, 32, generator=g)
        ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
        xd = x.to(dev)
        monkeypatch.setenv("DMET_KNN_PATH", "exact")
        n0, d0, _ = _knn_with_stats(xd, ptr, k)
        monkeypatch.delenv("DMET_KNN_PATH")
        n1, d1, st = _knn_with_stats(xd, ptr, k)
        assert torch.equal(n0, n1) and torch.equal(d0, d1), (it, sizes[:5], k, mode, st)


def test_knn_64_features_matrix_core_path(dev, monkeypatch):
    """K1 at the DRN's hidden width (model/dynamic_reduction_network.py:40,86: kNN in 64 features): events of 800+
    nodes go through the second filter form with 64-feature records, smaller ones and uncertified tiles through the
    exact kernel.  Bit-exact against the C oracle on one event, against the exact kernel on ragged / adversarial data."""
    from oracle import ref_ops
    g = torch.Generator().manual_seed(64)
    # (a) oracle: one 2300-node event + a small one (exact path inside the same call), k = 16 and the reference's k = 20
    sizes = [2300, 150]
    x = torch.randn(sum(sizes), 64, generator=g)
    x[700] = x[3]; x[701] = x[3]                                     # exact ties
    ptr = torch.tensor([0, 2300, 2450])
    for k in (16, 20):
        nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
        n1, d1, st = _knn_with_stats(x.to(dev), ptr.to(dev), k)
        assert torch.equal(n1, nbr_ref) and torch.equal(d1, dist_ref), (k, st)
    # (b) against the exact kernel: ragged sizes around the form's lower limit, clustered / heavy-tailed / offset data
    for it in range(6):
        sizes = [int(v) for v in torch.randint(1800 if it < 3 else 700, 5200 if it < 3 else 2400, (5,), generator=g)] + [0, 70]
        N = sum(sizes)
        x = torch.randn(N, 64, generator=g)
        if it % 3 == 1:
            c = torch.randn(5, 64, generator=g) * 3
            x = c[torch.randint(0, 5, (N,), generator=g)] + 1e-2 * torch.randn(N, 64, generator=g)
            x[N // 2:N // 2 + 200] = x[:200]
        elif it % 3 == 2:
            x = x * torch.exp(1.5 * torch.randn(N, 1, generator=g)) + (50.0 if it == 5 else 0.0)
        ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
        k = [16, 8, 20][it % 3]
        monkeypatch.setenv("DMET_KNN_PATH", "exact")
        n0, d0, _ = _knn_with_stats(x.to(dev), ptr, k)
        monkeypatch.delenv("DMET_KNN_PATH")
        n1, d1, st = _knn_with_stats(x.to(dev), ptr, k)
        assert torch.equal(n0, n1) and torch.equal(d0, d1), (it, sizes, k, st)


def test_radius_graph(dev):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    g = torch.Generator().manual_seed(3)
    sizes = [300, 5, 1000]
    N = sum(sizes)
    etaphi = torch.stack([(torch.rand(N, generator=g) - 0.5) * 6, (torch.rand(N, generator=g) - 0.5) * 6.28], 1)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    for loop, mx in [(True, 255), (False, 12), (True, 4)]:
        ref = ref_ops.radius_graph(etaphi, 0.4, batch, loop=loop, max_num_neighbors=mx)
        got = dm.radius_graph(etaphi.to(dev), 0.4, batch.to(dev), loop=loop, max_num_neighbors=mx)
        assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("case", ["etaphi", "dense_cluster", "one_d", "eight_d", "tiny_events", "nonfinite"])
def test_radius_windowed_equals_sweep(dev, monkeypatch, case):
    """N1: the radius table built with the first-coordinate window (dmet_radius_windowed_f32, the default) must be
    identical -- ids, order, counts -- to the all-pairs sweep (dmet_radius_f32, pinned to the oracle by
    test_radius_graph) on ragged batches, rows that overflow max_nbr, wavefronts that straddle events, 1-d / 8-d
    coordinates and non-finite coordinates."""
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(21)
    r, mx = 0.4, 255
    if case == "tiny_events":
        sizes = [int(v) for v in torch.randint(0, 40, (300,), generator=g)]
    else:
        sizes = [700, 0, 3, 1500, 64, 65, 129]
    N = sum(sizes)
    x = torch.stack([(torch.rand(N, generator=g) - 0.5) * 6, (torch.rand(N, generator=g) - 0.5) * 6.28], 1)
    if case == "dense_cluster":          # > 255 nodes within r of each other: "first max_nbr in index order" matters
        x[100:600] = x[100] + 0.05 * torch.randn(500, 2, generator=g)
        mx = 32
    elif case == "one_d":
        x = x[:, :1].contiguous()
    elif case == "eight_d":
        x = torch.cat([x, 0.1 * torch.randn(N, 6, generator=g)], 1).contiguous()
        r = 0.6
    elif case == "nonfinite":
        x[5, 0] = float("nan"); x[17, 1] = float("nan"); x[40, 0] = float("inf"); x[41, 0] = float("-inf")
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    xd = x.to(dev)
    for skip_self in (False, True):
        monkeypatch.setattr(_native, "RADIUS_FORM", "sweep")
        n0, c0 = _native.radius(xd, ptr, r, mx, skip_self=skip_self, pad=True)
        monkeypatch.setattr(_native, "RADIUS_FORM", "windowed")
        n1, c1 = _native.radius(xd, ptr, r, mx, skip_self=skip_self, pad=True)
        assert torch.equal(c0, c1), case
        assert torch.equal(n0, n1), case
    if case == "dense_cluster":
        assert int(c0.max()) == mx - 1 or int(c0.max()) == mx


def _close(a, b, rtol=FEAT_RTOL, atol=FEAT_ATOL):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)


@pytest.mark.parametrize("sizes,H,k", [([256], 32, 8), ([50, 450, 800], 32, 16), ([1, 3, 0, 17, 129], 32, 16),
                                        ([200, 100], 64, 20)])
def test_dynamic_edgeconv_fused_fwd_bwd(dev, sizes, H, k):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    x, batch, ptr = _ragged(sizes, H, seed=9 + H, dup=True)
    lin = torch.nn.Sequential(torch.nn.Linear(2 * H, H))
    conv = dm.DynamicEdgeConv(nn=lin, k=k)
    xr = x.clone().requires_grad_(True)
    out_ref = ref_ops.dynamic_edge_conv(xr, batch, lin, k)
    gup = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(1))
    out_ref.backward(gup)
    gW_ref, gb_ref, gx_ref = lin[0].weight.grad.clone(), lin[0].bias.grad.clone(), xr.grad.clone()
    lin.zero_grad()
    conv = conv.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, batch.to(dev))
    out.backward(gup.to(dev))
    _close(out.detach().cpu(), out_ref.detach())
    scale = float(gx_ref.abs().max())
    _close(xd.grad.cpu(), gx_ref, rtol=1e-4, atol=1e-5 * max(scale, 1.0))
    _close(lin[0].weight.grad.cpu(), gW_ref, rtol=1e-4, atol=1e-5 * float(gW_ref.abs().max()))
    _close(lin[0].bias.grad.cpu(), gb_ref, rtol=1e-4, atol=1e-5 * float(gb_ref.abs().max()))
    # residual-input form (graph_met_network.py:66, x + f(conv(x))): x handed through the conv's autograd node, its
    # second gradient added inside the backward kernel -- must equal the plain two-consumer graph
    lin.zero_grad()
    x2 = x.detach().clone().to(dev).requires_grad_(True)   # fresh leaf: on the CPU mirror of this test .to() aliases xd
    out2, res = conv.forward_with_residual_input(x2, batch.to(dev))
    gres = torch.randn(x.shape, generator=torch.Generator().manual_seed(2))
    (out2 * gup.to(dev)).sum().add((res * gres.to(dev)).sum()).backward()
    assert torch.equal(out2.detach(), out.detach()) and torch.equal(res.detach(), x2.detach())
    _close(x2.grad.cpu(), gx_ref + gres, rtol=1e-4, atol=1e-5 * max(scale, 1.0))
    _close(lin[0].weight.grad.cpu(), gW_ref, rtol=1e-4, atol=1e-5 * float(gW_ref.abs().max()))


@pytest.mark.parametrize("sizes,k", [([256], 8), ([50, 450, 800], 16), ([1, 3, 0, 17, 129], 16), ([300, 100], 32)])
def test_dynamic_edgeconv_bf16_mfma(dev, sizes, k):
    """BASELINE configs[2]: bf16 edge-MLP on the matrix cores.  (a) tight against a torch emulation of the same
    recipe (x, W1-W2, W2 rounded to bf16, fp32 accumulate, Q stored as bf16); (b) within the stated bf16 bar of
    the fp32 PyG-shaped oracle (rtol 2e-2); kNN stays fp32-exact; backward against the oracle's."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    H = 32
    x, batch, ptr = _ragged(sizes, H, seed=70 + k, dup=True)
    lin = torch.nn.Sequential(torch.nn.Linear(2 * H, H))
    conv = dm.DynamicEdgeConv(nn=lin, k=k)
    conv.compute_dtype = torch.bfloat16
    W, b = lin[0].weight.detach(), lin[0].bias.detach()
    xr = x.clone().requires_grad_(True)
    out_ref = ref_ops.dynamic_edge_conv(xr, batch, lin, k)
    gup = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(1))
    out_ref.backward(gup)
    gW_ref, gx_ref = lin[0].weight.grad.clone(), xr.grad.clone()
    lin.zero_grad()
    # emulation of the bf16 recipe on the oracle's graph
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    xb = bf(x)
    Pe = xb @ bf(W[:, :H] - W[:, H:]).t() + b
    Qe = bf(xb @ bf(W[:, H:]).t())
    nbr, _ = ref_ops.knn_table(x, ptr, k)
    g = Qe[nbr.long().clamp(min=0)]
    g = torch.where((nbr >= 0).unsqueeze(-1), g, torch.full_like(g, float("-inf")))
    emu = Pe + g.max(dim=1).values
    conv = conv.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, batch.to(dev))
    out.backward(gup.to(dev))
    o = out.detach().cpu()
    # (a) same recipe: only the accumulation order inside the MFMA and rare bf16 rounding flips of Q differ
    torch.testing.assert_close(o, emu, rtol=1e-2, atol=1e-2 * float(emu.abs().max()) * 2 ** -6)
    assert float((o - emu).abs().median()) < 1e-5 * max(1.0, float(emu.abs().max()))
    # (b) the stated bf16 bar against the fp32 oracle
    torch.testing.assert_close(o, out_ref.detach(), rtol=2e-2, atol=2e-2 * float(out_ref.abs().max()))
    # backward: fp32 arithmetic routed through the winners the bf16 table selected (straight-through over the
    # roundings).  Emulate exactly that: winners from the emulated table (lowest slot on ties), fp32 weights.
    valid = (nbr >= 0).unsqueeze(-1)
    slot = (g == g.max(dim=1, keepdim=True).values).float().argmax(dim=1)                  # [N,H] lowest winning slot
    src = torch.gather(nbr.long().clamp(min=0), 1, slot)                                   # [N,H] winning source node
    gQ = torch.zeros_like(Qe)
    gQ.scatter_add_(0, src, gup)
    Wd, W2 = W[:, :H] - W[:, H:], W[:, H:]
    gx_emu = gup @ Wd + gQ @ W2
    gWd, gW2 = gup.t() @ x, gQ.t() @ x
    gW_emu = torch.cat([gWd, gW2 - gWd], dim=1)
    rel = float((xd.grad.cpu() - gx_emu).norm() / gx_emu.norm())
    assert rel < 2e-2, rel          # a rare bf16 rounding flip of Q moves one winner; everything else is fp32-exact
    relw = float((lin[0].weight.grad.cpu() - gW_emu).norm() / gW_emu.norm())
    assert relw < 2e-2, relw
    # and the routing error w.r.t. the fp32 oracle stays bounded (near-ties decided differently by bf16)
    assert float((xd.grad.cpu() - gx_ref).norm() / gx_ref.norm()) < 0.5


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
def test_edgeconv_generic_nn_irregular_graph(dev, aggr):
    """DRN call shape (dynamic_reduction_network.py:59-73,86-87): multi-layer nn, loop=False kNN, symmetrised
    (irregular, unsorted) edge_index handed to EdgeConv."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    x, batch, ptr = _ragged([60, 5, 90], 16, seed=21)
    nn_ = torch.nn.Sequential(torch.nn.Linear(32, 24), torch.nn.ELU(), torch.nn.Linear(24, 16), torch.nn.ELU())
    conv = dm.EdgeConv(nn=nn_, aggr=aggr)        # like PyG, construction re-initialises nn: build it first
    ei = ref_ops.knn_graph(x, 4, batch, loop=False)
    ei = torch.cat([ei, ei.flip(0)], dim=1)                     # to_undirected-like (duplicates allowed), unsorted
    ei = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(0))]
    xr = x.clone().requires_grad_(True)
    out_ref = ref_ops.edge_conv(xr, ei, nn_, aggr)
    gup = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(2))
    out_ref.backward(gup)
    gx_ref = xr.grad.clone()
    gw_ref = nn_[0].weight.grad.clone()
    nn_.zero_grad()
    conv = conv.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev))
    out.backward(gup.to(dev))
    _close(out.detach().cpu(), out_ref.detach(), rtol=1e-4, atol=1e-5)
    _close(xd.grad.cpu(), gx_ref, rtol=1e-4, atol=1e-5 * max(1.0, float(gx_ref.abs().max())))
    _close(nn_[0].weight.grad.cpu(), gw_ref, rtol=1e-4, atol=1e-5 * max(1.0, float(gw_ref.abs().max())))


def test_edgeconv_static_graph_from_radius(dev):
    """The active reference flow (train.py:48-49): radius_graph -> EdgeConv(Linear) with variable degree."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    g = torch.Generator().manual_seed(4)
    N = 500
    etaphi = torch.rand(N, 2, generator=g) * 3
    emb = torch.randn(N, 32, generator=g)
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor([200, 300]))
    lin = torch.nn.Sequential(torch.nn.Linear(64, 32))
    conv = dm.EdgeConv(nn=lin).jittable()
    ref = ref_ops.edge_conv(emb, ref_ops.radius_graph(etaphi, 0.4, batch, loop=True, max_num_neighbors=255), lin)
    conv = conv.to(dev)
    ei = dm.radius_graph(etaphi.to(dev), 0.4, batch.to(dev), loop=True, max_num_neighbors=255)
    out = conv(emb.to(dev), ei)
    _close(out.detach().cpu(), ref.detach())
    # the table itself instead of the [2,E] tensor (no host-side edge count): same graph, same bits
    table = dm.radius_table(etaphi.to(dev), 0.4, batch.to(dev), loop=True, max_num_neighbors=255)
    assert torch.equal(conv(emb.to(dev), table), out)
    assert torch.equal(table.edge_index("source_to_target"), ei)


def test_edgeconv_radius_backward_with_nonfinite_coordinates(dev):
    """Round 3 (advisor finding): a query with a NaN / inf coordinate finds nobody, not even itself, although the table
    was built with self loops -- its row is empty, its output 0 (R3) and NO gradient may reach the dense layer through
    it.  The winner-id form of the counted gather (the default of the static flow) used to skip that mask."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    g = torch.Generator().manual_seed(14)
    sizes = [220, 300]
    N = sum(sizes)
    etaphi = torch.rand(N, 2, generator=g) * 3
    etaphi[5, 0] = float("nan")
    etaphi[17, 1] = float("inf")
    etaphi[250, 0] = float("-inf")
    etaphi[N - 1] = float("nan")
    emb = torch.randn(N, 32, generator=g)
    gup = torch.randn(N, 32, generator=g)
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes))
    lin = torch.nn.Sequential(torch.nn.Linear(64, 32))
    conv = dm.EdgeConv(nn=lin)          # (the constructor resets the parameters of nn, like PyG's: build it first)
    ei_ref = ref_ops.radius_graph(etaphi, 0.4, batch, loop=True, max_num_neighbors=255)
    xr = emb.clone().requires_grad_(True)
    ref = ref_ops.edge_conv(xr, ei_ref, lin)
    ref.backward(gup)
    gw_ref, gb_ref, gx_ref = lin[0].weight.grad.clone(), lin[0].bias.grad.clone(), xr.grad.clone()
    lin.zero_grad()
    assert bool((ref[[5, 17, 250, N - 1]] == 0).all())
    conv = conv.to(dev)
    table = dm.radius_table(etaphi.to(dev), 0.4, batch.to(dev), loop=True, max_num_neighbors=255)
    assert torch.equal(table.edge_index("source_to_target").cpu(), ei_ref)
    xd = emb.to(dev).requires_grad_(True)
    out = conv(xd, table)
    out.backward(gup.to(dev))
    _close(out.detach().cpu(), ref.detach())
    _close(xd.grad.cpu(), gx_ref, rtol=1e-4, atol=1e-5 * max(1.0, float(gx_ref.abs().max())))
    _close(lin[0].weight.grad.cpu(), gw_ref, rtol=1e-4, atol=1e-5 * max(1.0, float(gw_ref.abs().max())))
    _close(lin[0].bias.grad.cpu(), gb_ref, rtol=1e-4, atol=1e-5 * max(1.0, float(gb_ref.abs().max())))


@pytest.mark.parametrize("reverse_route", [False, True])
def test_counted_radius_table_consumers_go_by_cnt(dev, monkeypatch, reverse_route):
    """N1: radius tables are built WITHOUT the -1 fill of their unused slots (dmet_radius_counted_f32).  Every consumer
    must go by cnt: the same table with its undefined slots overwritten by a valid but wrong node id has to give the
    same edge_index, the same EdgeConv output and the same gradients (both backward routes)."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, conv as conv_mod
    from deepmetv2_amd.graph import NeighborTable
    if reverse_route:
        monkeypatch.setattr(conv_mod, "GATHER_BWD_FORM", "reverse")
    g = torch.Generator().manual_seed(8)
    sizes = [200, 0, 300, 1]
    N = sum(sizes)
    etaphi = (torch.rand(N, 2, generator=g) * 3).to(dev)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    nbr_p, cnt_p = _native.radius(etaphi, ptr, 0.4, 255, skip_self=False, pad=True)
    nbr_u, cnt_u = _native.radius(etaphi, ptr, 0.4, 255, skip_self=False, pad=False)
    assert torch.equal(cnt_p, cnt_u)
    slot = torch.arange(255, device=dev, dtype=torch.int32).view(1, -1)
    live = slot < cnt_p.view(-1, 1)
    assert torch.equal(nbr_p[live], nbr_u[live]) and bool((nbr_p[~live] == -1).all())
    nbr_u = torch.where(live, nbr_u, torch.zeros_like(nbr_u))           # poison: node 0 everywhere it is undefined
    lin = torch.nn.Sequential(torch.nn.Linear(64, 32)).to(dev)
    conv = dm.EdgeConv(nn=lin)
    emb = torch.randn(N, 32, generator=g).to(dev)
    gup = torch.randn(N, 32, generator=g).to(dev)
    res = []
    for nbr in (nbr_p, nbr_u):
        table = NeighborTable(nbr, ptr, dense=False, max_nodes=max(sizes), cnt=cnt_p)
        x = emb.clone().requires_grad_(True)
        lin.zero_grad()
        out = conv._forward_table(x, table)
        out.backward(gup)
        res.append((out.detach(), x.grad.clone(), lin[0].weight.grad.clone(), table.edge_index("source_to_target")))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    if not reverse_route:   # LDS-resident and L2 forms of the counted gather give the same bits (+ an oversized event)
        Pm = torch.randn(N, 32, generator=g).to(dev)
        Qm = torch.randn(N, 32, generator=g).to(dev)
        for want_arg in (True, False):
            o0, a0 = _native.gather_max(Pm, Qm, nbr_u, ptr, want_arg, cnt=cnt_p, lds=False)
            o1, a1 = _native.gather_max(Pm, Qm, nbr_u, ptr, want_arg, cnt=cnt_p, lds=True)
            assert torch.equal(o0, o1) and (not want_arg or torch.equal(a0, a1))
        big = [5300, 40]
        xb = (torch.rand(sum(big), 2, generator=g) * torch.tensor([40.0, 6.0])).to(dev)
        pb = torch.tensor([0, 5300, 5340], device=dev)
        nb, cb = _native.radius(xb, pb, 0.4, 255, pad=False)
        Pb = torch.randn(sum(big), 32, generator=g).to(dev)
        Qb = torch.randn(sum(big), 32, generator=g).to(dev)
        o0, a0 = _native.gather_max(Pb, Qb, nb, pb, True, cnt=cb, lds=False)
        o1, a1 = _native.gather_max(Pb, Qb, nb, pb, True, cnt=cb, lds=True)
        assert torch.equal(o0, o1) and torch.equal(a0, a1)
        # slice-major P / Q through the counted LDS kernel (small events, then the oversized one); not under
        # DMET_GATHER_MAX_FORM=l2-only, which has no reader for that layout
        for Pr, Qr, tb, pp, cc in (((Pm, Qm, nbr_u, ptr, cnt_p), (Pb, Qb, nb, pb, cb))
                                   if _native.GATHER_MAX_FORM != "l2-only" else ()):
            Ps = Pr.view(-1, 4, 8).permute(1, 0, 2).contiguous()
            Qs = Qr.view(-1, 4, 8).permute(1, 0, 2).contiguous()
            o0, a0 = _native.gather_max(Pr, Qr, tb, pp, True, cnt=cc, lds=True)
            o1, a1 = _native.gather_max(Ps, Qs, tb, pp, True, cnt=cc, lds=True, sliced=True)
            assert torch.equal(o0, o1) and torch.equal(a0, a1)


@pytest.mark.parametrize("sizes", [[300, 1, 0, 77], [1152, 1100, 5], [2304, 1153], [4700, 50], [9500], [19000, 3]])
def test_gather_max_bwd_lds_matches_reverse_index_route(dev, sizes):
    """K5: the LDS fixed-point scatter (no reverse index) against the sorted reverse-index kernel (itself pinned to
    the oracle by the EdgeConv backward tests): 1e-6 of max|g| per cell (each term is rounded to 2^-30 of the
    slice maximum), bitwise reproducible, all window shapes (4 / 2 / 1 channels, several j windows)."""
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(sum(sizes))
    N, k, H = sum(sizes), 16, 32
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)])
    nbr = torch.empty(N, k, dtype=torch.int32)
    for b, n in enumerate(sizes):
        if n:
            lo = int(ptr[b])
            # skewed in-degrees: half of the slots point at the first 5 nodes of the event
            r = torch.randint(0, n, (n, k), generator=g)
            hot = torch.randint(0, min(n, 5), (n, k), generator=g)
            nbr[lo:lo + n] = (torch.where(torch.rand(n, k, generator=g) < 0.5, hot, r) + lo).int()
    arg = torch.randint(0, k, (N, H), generator=g).to(torch.uint8)
    arg[::7, 3] = 255
    g_out = torch.randn(N, H, generator=g) * torch.logspace(-3, 2, H)
    nd, ad, gd, pd = nbr.to(dev), arg.to(dev), g_out.to(dev), ptr.to(dev)
    rev_ptr, rev_pos = _native.reverse_index(nd.view(-1), N)
    ref = _native.gather_max_bwd(gd, ad, rev_ptr, rev_pos, k)
    got = _native.gather_max_bwd_lds(gd, ad, nd, pd)
    got2 = _native.gather_max_bwd_lds(gd, ad, nd, pd)
    assert torch.equal(got, got2)
    # the uint16 event-local table gives the same bits (integer sums)
    lo = torch.repeat_interleave(ptr[:-1], torch.tensor(sizes)).to(torch.int32).view(-1, 1)
    loc = nbr - lo
    loc = torch.where(loc >= 0x8000, loc - 0x10000, loc).to(torch.int16).to(dev)
    assert torch.equal(got, _native.gather_max_bwd_lds(gd, ad, nd, pd, nbr_local=loc))
    # the hint on the largest event only sizes the workgroups (256 / 512 / 1024 threads): same bits for a true hint, for
    # one that is too small (more passes over the window) and for one that is too large
    for hint in (max(sizes), 1000, 2304, 2305, 100000):
        assert torch.equal(got, _native.gather_max_bwd_lds(gd, ad, nd, pd, nbr_local=loc, max_nodes=hint)), hint
        assert torch.equal(got, _native.gather_max_bwd_lds(gd, ad, nd, pd, max_nodes=hint)), hint
    scale = g_out.abs().amax(0).to(dev) * float(max(sizes)) * 1e-6 + 1e-12
    assert bool(((got - ref).abs() <= scale + 1e-5 * ref.abs()).all())


@pytest.mark.parametrize("sizes", [[4609, 20], [6000, 9216, 300], [9217, 4608]])
def test_gather_max_bwd_winner_id_form_at_large_events(dev, sizes):
    """K5, winner-id form (dmet_gather_max_bwd_j16_f32) around the window boundaries of the LDS scatter: events of
    4 609 .. 9 216 nodes take the two-pass / one-look-up path, larger ones the one-channel windows.  Against the slot
    form on the same winners (integer sums: bit for bit) and against a float64 index_add (1e-6 of max|g| x in-degree)."""
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(sum(sizes))
    N, k, H = sum(sizes), 16, 32
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)])
    lo = torch.repeat_interleave(ptr[:-1], torch.tensor(sizes)).view(-1, 1)
    cnt = torch.repeat_interleave(torch.tensor(sizes), torch.tensor(sizes)).view(-1, 1)
    nbr = (lo + (torch.rand(N, k, generator=g) * cnt).long().clamp_(max=int(max(sizes)) - 1)).to(torch.int32)
    nbr = torch.minimum(nbr, (lo + cnt - 1).to(torch.int32))
    arg = torch.randint(0, k, (N, H), generator=g).to(torch.uint8)
    arg[::5, 1] = 255
    arg[3::11, 30] = 255
    g_out = torch.randn(N, H, generator=g) * torch.logspace(-2, 2, H)
    win = torch.gather(nbr.long(), 1, arg.long().clamp(max=k - 1)) - lo           # event-local winner ids
    argj = torch.where(arg == 255, torch.full_like(win, 0xFFFF), win)
    argj16 = torch.where(argj >= 0x8000, argj - 0x10000, argj).to(torch.int16)
    pd, gd = ptr.to(dev), g_out.to(dev)
    got = _native.gather_max_bwd_j16(gd, argj16.to(dev), pd)
    assert torch.equal(got, _native.gather_max_bwd_j16(gd, argj16.to(dev), pd))
    for hint in (max(sizes), 900, 2000):          # workgroup size hint: true, and far too small
        assert torch.equal(got, _native.gather_max_bwd_j16(gd, argj16.to(dev), pd, max_nodes=hint)), hint
    slot_form = _native.gather_max_bwd_lds(gd, arg.to(dev), nbr.to(dev), pd)
    assert torch.equal(got, slot_form)
    ref = torch.zeros(N, H, dtype=torch.float64)
    tgt = (win + lo).clamp(0, N - 1)
    gm = torch.where(arg == 255, torch.zeros(()), g_out).double()
    ref.scatter_add_(0, tgt, gm)
    indeg = torch.zeros(N, H).scatter_add_(0, tgt, (arg != 255).float()).amax()
    tol = g_out.abs().amax(0).double() * float(indeg) * 1e-6 + 1e-12
    assert bool(((got.cpu().double() - ref).abs() <= tol + 1e-6 * ref.abs()).all())


@pytest.mark.parametrize("k", [8, 16, 20, 32])
def test_gather_max_local_ids_kernel_matches(dev, k):
    """K3: the LDS gather kernel fed with the uint16 event-local table must return the bits of the int32 form (and
    of the L2 form), including an event too large for the LDS image (reads the int32 table) and empty events."""
    from deepmetv2_amd import _native
    _default_path_only("DMET_GATHER_MAX_FORM", "l2-only", "the slice-major / LDS-resident forms compared here are switched off "
                       "(gather_max raises ValueError for slice-major tables by design)")
    sizes = [300, 1, 0, 77, 5200, 4500]
    x, batch, ptr = _ragged(sizes, 32, seed=11 + k)
    xd, ptrd = x.to(dev), ptr.to(dev)
    nbr, _, loc = _native.knn_local(xd, ptrd, k)
    _check_local_table(nbr, loc, ptrd)
    g = torch.Generator().manual_seed(3)
    P = torch.randn(x.shape[0], 32, generator=g).to(dev)
    Q = torch.randn(x.shape[0], 32, generator=g).to(dev)
    for want_arg in (True, False):
        o0, a0 = _native.gather_max(P, Q, nbr, ptrd, want_arg, lds=False)
        o1, a1 = _native.gather_max(P, Q, nbr, ptrd, want_arg, lds=True)
        o2, a2 = _native.gather_max(P, Q, nbr, ptrd, want_arg, lds=True, nbr_local=loc)
        assert torch.equal(o0, o1) and torch.equal(o1, o2)
        if want_arg:
            assert torch.equal(a0, a1) and torch.equal(a1, a2)
    # slice-major P / Q ([H/8][N][8], dmet_node_linear_split_sliced_f32 -> dmet_gather_max_lds_sliced_f32): same bits as
    # the row-major pair, with and without the uint16 table, oversized event included
    W = (torch.randn(32, 64, generator=g) * 0.2).to(dev)
    b = torch.randn(32, generator=g).to(dev)
    Pr, Qr = _native.node_linear_split(xd, W, b)
    Ps, Qs = _native.node_linear_split(xd, W, b, sliced=True)
    assert Ps.shape == (4, x.shape[0], 8)
    assert torch.equal(Ps.permute(1, 0, 2).reshape(-1, 32), Pr) and torch.equal(Qs.permute(1, 0, 2).reshape(-1, 32), Qr)
    for want_arg in (True, False):
        o0, a0 = _native.gather_max(Pr, Qr, nbr, ptrd, want_arg, lds=True, nbr_local=loc)
        for nl in (loc, None):
            o1, a1 = _native.gather_max(Ps, Qs, nbr, ptrd, want_arg, lds=True, nbr_local=nl, sliced=True)
            assert torch.equal(o0, o1) and (not want_arg or torch.equal(a0, a1))


def test_gather_max_work_mappings_agree(dev, monkeypatch):
    """K3: the LDS gather kernel's two block -> work mappings (one workgroup per (event, slice); one workgroup per CU
    walking equal ranges of the [event][slice][node] axis, whose boundaries cut events and slices) must give the
    same bits on a ragged batch with empty, tiny and oversized events, for both table forms and P / Q layouts."""
    from deepmetv2_amd import _native
    _default_path_only("DMET_GATHER_MAX_FORM", "l2-only", "both mappings under test belong to the LDS-resident kernel")
    sizes = [1900, 0, 3, 4800, 64, 5150, 1, 2500, 700]
    x, batch, ptr = _ragged(sizes, 32, seed=21)
    xd, ptrd = x.to(dev), ptr.to(dev)
    nbr, _, loc = _native.knn_local(xd, ptrd, 16)
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(32, 64, generator=g) * 0.2).to(dev)
    b = torch.randn(32, generator=g).to(dev)
    for sliced in (False, True):
        P, Q = _native.node_linear_split(xd, W, b, sliced=sliced)
        for nl in (loc, None):
            res = {}
            for mode in ("0", "1"):
                monkeypatch.setenv("DMET_GATHER_BALANCED", mode)
                res[mode] = _native.gather_max(P, Q, nbr, ptrd, True, lds=True, nbr_local=nl, sliced=sliced)
            monkeypatch.delenv("DMET_GATHER_BALANCED")
            assert torch.equal(res["0"][0], res["1"][0]) and torch.equal(res["0"][1], res["1"][1])


def test_max_ties_and_empty_rows(dev):
    """R3: empty target -> 0.  R4: gradient to the lowest edge position among exact ties."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    src = torch.tensor([[1.0, 5.0], [1.0, 5.0], [0.5, 7.0], [2.0, 2.0]], requires_grad=True)
    index = torch.tensor([0, 0, 0, 3])
    out_ref, arg_ref = ref_ops.scatter_max(src, index, 5)
    out_ref.sum().backward()
    g_ref = src.grad.clone()
    sd = src.detach().to(dev).requires_grad_(True)
    out, arg = dm.scatter_max(sd, index.to(dev), dim=0, dim_size=5)
    out.sum().backward()
    assert torch.equal(out.detach().cpu(), out_ref.detach())
    assert torch.equal(arg.cpu(), arg_ref)
    assert torch.equal(sd.grad.cpu(), g_ref)


def test_met_reduce_and_scatter_add(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from oracle import ref_ops
    x, y, batch, ptr = synth.make_events([4500, 1, 0, 777, 8000], seed=5)
    w = torch.rand(x.shape[0], generator=torch.Generator().manual_seed(8))
    ref = ref_ops.met_sums_f64(w, x, ptr)
    mag = torch.zeros(5, 2, dtype=torch.float64)
    mag.index_add_(0, batch, (w.view(-1, 1) * x[:, :2]).abs().double())
    xd, wd, bd = x.to(dev), w.to(dev).requires_grad_(True), batch.to(dev)
    met = dm.met_reduce(wd, xd, bd, num_events=5)
    assert bool(((met.detach().cpu().double() - ref).abs() <= 1e-5 * mag + 1e-12).all())
    sx = dm.scatter_add(wd * xd[:, 0], bd, dim_size=5)
    sy = dm.scatter_add(wd * xd[:, 1], bd)                       # dim_size inferred, like net.py:55-56
    assert sy.shape == (5,)
    assert bool(((torch.stack([sx, sy], 1).detach().cpu().double() - ref).abs() <= 1e-5 * mag + 1e-12).all())
    # run-to-run determinism (no float atomics)
    assert torch.equal(met, dm.met_reduce(wd, xd, bd, num_events=5))
    # backward: d/dw of sum_b (a_b*METx + c_b*METy)
    coef = torch.randn(5, 2, generator=torch.Generator().manual_seed(1))
    (met * coef.to(dev)).sum().backward()
    g_ref = coef[batch, 0] * x[:, 0] + coef[batch, 1] * x[:, 1]
    torch.testing.assert_close(wd.grad.cpu(), g_ref, rtol=1e-6, atol=1e-6)


def test_full_model_train_step_matches_oracle(dev):
    """H1/H2: Net(dynamic kNN, k=16) forward + loss + backward on a ragged seeded batch vs the oracle model."""
    import deepmetv2_amd as dm  # noqa: F401
    from deepmetv2_amd import synth
    from deepmetv2_amd.model import Net, loss_fn, split_features
    from oracle import ref_model, ref_ops
    torch.manual_seed(3)
    x, y, batch, ptr = synth.make_events([600, 40, 1100], seed=21)
    model = Net(8, 3, graph="dynamic", k=16)
    ref = ref_model.RefNet(8, 3, graph="dynamic", k=16)
    ref.load_state_dict(model.state_dict())
    model.to(dev).train(); ref.train()
    xd, yd, bd = x.to(dev), y.to(dev), batch.to(dev)
    w = model(*split_features(xd), None, bd)
    loss = loss_fn(w, xd, yd, bd)
    loss.backward()
    w_ref = ref(*split_features(x), None, batch)
    loss_ref = ref_ops.loss_fn(w_ref, x, y, batch)
    loss_ref.backward()
    torch.testing.assert_close(w.detach().cpu(), w_ref.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(loss.detach().cpu(), loss_ref.detach(), rtol=1e-4, atol=1e-3)
    # absolute floor from the global gradient scale: biases in front of a train-mode BatchNorm have an exactly-zero
    # true gradient, what is left in both implementations is cancellation noise of that scale
    gscale = max(float(q.grad.abs().max()) for q in ref.parameters())
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        torch.testing.assert_close(p.grad.cpu(), q.grad, rtol=2e-3, atol=2e-4 * gscale,
                                   msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("N,Ha,Hb", [(1, 1, 16), (1000, 16, 8), (4097, 32, 32), (70001, 16, 24), (5000, 64, 33)])
def test_dense_weight_grad_kernels(dev, N, Ha, Hb):
    """csrc/dense.hip: A^T B and onehot(index)^T B vs an fp64 reference; deterministic run to run."""
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(N)
    A, Bm = torch.randn(N, Ha, generator=g), torch.randn(N, Hb, generator=g)
    ref = (A.double().t() @ Bm.double())
    got = _native.xty(A.to(dev), Bm.to(dev))
    tol = 1e-5 * float((A.abs().double().t() @ Bm.abs().double()).max())
    assert float((got.cpu().double() - ref).abs().max()) <= tol
    assert torch.equal(got, _native.xty(A.to(dev), Bm.to(dev)))
    R = min(Ha, 8)
    idx = torch.randint(0, R, (N,), generator=g)
    ref2 = torch.zeros(R, Hb, dtype=torch.float64).index_add_(0, idx, Bm.double())
    got2 = _native.onehot_xty(idx.to(dev), Bm.to(dev), R)
    assert float((got2.cpu().double() - ref2).abs().max()) <= 1e-5 * max(1.0, float(ref2.abs().max()))


@pytest.mark.parametrize("N", [1, 63, 65, 5000, 70001])
def test_fused_encoder_fwd_bwd(dev, N):
    """N3: csrc/encoder.hip (one kernel each way) vs the oracle's layer-by-layer encoder in float64 on the CPU
    (the restatement of graph_met_network.py:48-58 in oracle/ref_model.py), including unexpected pdg ids."""
    from deepmetv2_amd import dense
    from per_node_reference import ENCODER_PARAM_NAMES as names, encoder_inputs, encoder_params, encoder_ref
    x_cont, x_cat, g_h = encoder_inputs(N, seed=N)
    cpu_params = encoder_params(seed=11)
    # reference chain in float64
    h_ref, leaves = encoder_ref(x_cont, x_cat, cpu_params, g_h)
    params = [p.to(dev).requires_grad_(True) for p in cpu_params]
    big = torch.cat([x_cont, x_cat.float()], dim=1).to(dev)          # strided view, as split_features hands over
    h = dense.encode(big[:, :8], x_cat.to(dev), *params)
    h.backward(g_h.to(dev))
    torch.testing.assert_close(h.detach().cpu().double(), h_ref.detach(), rtol=1e-5, atol=1e-5)
    for n, p, leaf in zip(names, params, leaves):
        r = leaf.grad
        torch.testing.assert_close(p.grad.cpu().double(), r, rtol=1e-4, atol=1e-5 * max(1.0, float(r.abs().max())),
                                   msg=lambda m, n=n: f"{n}: {m}")
    # bitwise reproducible (fixed reduction order)
    params2 = [p.detach().clone().requires_grad_(True) for p in params]
    dense.encode(big[:, :8], x_cat.to(dev), *params2).backward(g_h.to(dev))
    for p, q in zip(params, params2):
        assert torch.equal(p.grad, q.grad)
    # categorical columns handed over as the float view of the same rows (split_features(x, lazy_cat=True)): the
    # kernel does the `.long()` of train.py:43 itself -- same bits
    params3 = [p.detach().clone().requires_grad_(True) for p in params]
    h3 = dense.encode(big[:, :8], big[:, 8:], *params3)
    h3.backward(g_h.to(dev))
    assert torch.equal(h3, h)
    for p, q in zip(params, params3):
        assert torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("N,H,residual,training", [(5000, 32, True, True), (70001, 32, False, True), (3, 8, True, True),
                                                   (1000, 64, True, False), (4097, 16, False, True)])
def test_batch_norm_residual_fwd_bwd(dev, N, H, residual, training):
    """N3: csrc/norm.hip vs torch.nn.BatchNorm1d in float64 on the CPU (same module state, running statistics
    included), with a large common offset in x to exercise the shifted-sum statistics."""
    from deepmetv2_amd import dense
    g = torch.Generator().manual_seed(N + H)
    x = torch.randn(N, H, generator=g) * 0.7 + 3.0
    r = torch.randn(N, H, generator=g) if residual else None
    gup = torch.randn(N, H, generator=g)
    ref = torch.nn.BatchNorm1d(H).double()
    with torch.no_grad():
        ref.weight.copy_(torch.rand(H, generator=g) + 0.5); ref.bias.copy_(torch.randn(H, generator=g))
        ref.running_mean.copy_(torch.randn(H, generator=g)); ref.running_var.copy_(torch.rand(H, generator=g) + 0.5)
    bn = torch.nn.BatchNorm1d(H)
    bn.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
    bn = bn.to(dev)
    ref.train(training); bn.train(training)
    x64 = x.double().requires_grad_(True)
    r64 = r.double().requires_grad_(True) if residual else None
    y_ref = ref(x64) + (r64 if residual else 0.0)
    y_ref.backward(gup.double())
    xd = x.to(dev).requires_grad_(True)
    rd = r.to(dev).requires_grad_(True) if residual else None
    y = dense.batch_norm(xd, bn, residual=rd)
    y.backward(gup.to(dev))
    torch.testing.assert_close(y.detach().cpu().double(), y_ref.detach(), rtol=2e-5, atol=2e-5)
    gs = float(x64.grad.abs().max())
    torch.testing.assert_close(xd.grad.cpu().double(), x64.grad, rtol=1e-4, atol=2e-5 * max(gs, 1.0))
    if residual:
        assert torch.equal(rd.grad.cpu(), gup)
    torch.testing.assert_close(bn.weight.grad.cpu().double(), ref.weight.grad, rtol=1e-4,
                               atol=1e-5 * max(1.0, float(ref.weight.grad.abs().max())))
    torch.testing.assert_close(bn.bias.grad.cpu().double(), ref.bias.grad, rtol=1e-4,
                               atol=1e-5 * max(1.0, float(ref.bias.grad.abs().max())))
    torch.testing.assert_close(bn.running_mean.cpu().double(), ref.running_mean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(bn.running_var.cpu().double(), ref.running_var, rtol=1e-5, atol=1e-5)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)


@pytest.mark.parametrize("N,H,residual", [(5000, 32, True), (70001, 32, False), (3, 8, True), (1000, 64, False)])
def test_batch_norm_apply_alone_has_the_bits_of_bn_fwd(dev, N, H, residual):
    """dmet_bn_apply_f32 (the transform with the statistics given: what a caller runs when its fused consumer declined
    after the statistics were computed) = dmet_bn_fwd_f32 bit for bit, training and eval statistics, also with the
    small vectors sitting at odd offsets of a flat buffer."""
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(7 * N + H)
    x = (torch.randn(N, H, generator=g) * 0.7 + 3.0).to(dev)
    r = torch.randn(N, H, generator=g).to(dev) if residual else None
    flat = torch.randn(4 * H + 3, generator=g).to(dev)          # gamma / beta at 4-byte offsets 1 and H + 2
    gamma, beta = flat[1:1 + H], flat[H + 2:2 * H + 2]
    assert gamma.data_ptr() % 16 != 0
    rm, rv = torch.randn(H, generator=g).to(dev), (torch.rand(H, generator=g) + 0.5).to(dev)
    for training in (True, False):
        y_ref, mean, invstd = _native.bn_fwd(x, r, gamma.clone(), beta.clone(), 1e-5, 0.1, rm.clone(), rv.clone(), training)
        if training:
            m2, i2 = _native.bn_stats(x, 1e-5, 0.1, rm.clone(), rv.clone())
        else:
            m2, i2 = _native.bn_eval_stats(rm, rv, 1e-5)
        assert torch.equal(m2, mean) and torch.equal(i2, invstd)
        y = _native.bn_apply(x, r, gamma, beta, m2, i2)
        assert torch.equal(y, y_ref)


@pytest.mark.parametrize("N", [1, 64, 65, 5000, 70001])
def test_fused_head_fwd_bwd(dev, N):
    """N3: csrc/head.hip vs sigmoid(Linear(ELU(Linear(emb)))) in float64 on the CPU."""
    from deepmetv2_amd import dense
    g = torch.Generator().manual_seed(N)
    emb = torch.randn(N, 32, generator=g)
    W1, b1 = torch.randn(16, 32, generator=g) * 0.3, torch.randn(16, generator=g) * 0.3
    W2, b2 = torch.randn(1, 16, generator=g) * 0.5, torch.randn(1, generator=g)
    gup = torch.randn(N, generator=g)
    F = torch.nn.functional
    ref = [t.double().requires_grad_(True) for t in (emb, W1, b1, W2, b2)]
    o_ref = torch.sigmoid(F.linear(F.elu(F.linear(ref[0], ref[1], ref[2])), ref[3], ref[4])).squeeze(-1)
    o_ref.backward(gup.double())
    got = [t.to(dev).requires_grad_(True) for t in (emb, W1, b1, W2, b2)]
    o = dense.head(*got)
    o.backward(gup.to(dev))
    torch.testing.assert_close(o.detach().cpu().double(), o_ref.detach(), rtol=1e-5, atol=1e-6)
    for a, r, name in zip(got, ref, ["emb", "W1", "b1", "W2", "b2"]):
        torch.testing.assert_close(a.grad.cpu().double(), r.grad, rtol=1e-4,
                                   atol=1e-5 * max(1.0, float(r.grad.abs().max())), msg=lambda m, n=name: f"{n}: {m}")
    got2 = [t.detach().clone().requires_grad_(True) for t in got]
    dense.head(*got2).backward(gup.to(dev))
    for a, b in zip(got, got2):
        assert torch.equal(a.grad, b.grad)


def test_dense_linear_embedding_autograd(dev):
    from deepmetv2_amd import dense
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3000, 24, generator=g)
    W, b = torch.randn(16, 24, generator=g), torch.randn(16, generator=g)
    tab = torch.randn(7, 8, generator=g)
    idx = torch.randint(0, 7, (3000,), generator=g)
    outs = []
    for d in (torch.device("cpu"), dev):
        xx, WW, bb, tt = (t.clone().to(d).requires_grad_(True) for t in (x, W, b, tab))
        if d.type == "cpu":
            y = torch.nn.functional.linear(xx, WW, bb).tanh().sum() + (torch.nn.functional.embedding(idx, tt) ** 2).sum()
        else:
            y = dense.linear(xx, WW, bb).tanh().sum() + (dense.embedding(idx.to(d), tt) ** 2).sum()
        y.backward()
        outs.append([t.grad.cpu() for t in (xx, WW, bb, tt)])
    for a, r in zip(outs[1], outs[0]):
        torch.testing.assert_close(a, r, rtol=1e-4, atol=1e-4 * max(1.0, float(r.abs().max())))


def test_training_trajectory_matches_oracle(dev):
    """H1: 8 AdamW steps of `parallel.train_step` (FlatModule + gather_grads + optimizer on the flat vector) against the
    oracle model trained with stock torch on the CPU: losses, final parameters and BatchNorm running statistics."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from deepmetv2_amd.model import Net
    from deepmetv2_amd.parallel import FlatModule, GradSync, train_step
    from oracle import ref_model, ref_ops
    sizes = [300, 40, 500]
    x, y, batch, ptr = synth.make_events(sizes, seed=77)
    torch.manual_seed(5)
    model = Net(8, 3, graph="dynamic", k=16)
    ref = ref_model.RefNet(8, 3, graph="dynamic", k=16)
    ref.load_state_dict(model.state_dict())
    model.to(dev).train(); ref.train()
    xd, yd, bd, pd = x.to(dev), y.to(dev), batch.to(dev), ptr.to(dev)
    dm.register_batch(bd, pd, len(sizes), max_nodes=max(sizes))
    flat = FlatModule(model); sync = GradSync(flat)
    opt = torch.optim.AdamW([flat.flat_param], lr=1e-3)
    opt_ref = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    losses, losses_ref = [], []
    for _ in range(8):
        losses.append(float(train_step(model, flat, sync, opt, xd, yd, bd, pd)))
        opt_ref.zero_grad()
        lr_ = ref_ops.loss_fn(ref(x[:, :8], x[:, 8:].long(), None, batch), x, y, batch)
        lr_.backward(); opt_ref.step()
        losses_ref.append(float(lr_.detach()))
    for a, b in zip(losses, losses_ref):
        assert abs(a - b) <= 2e-4 * abs(b) + 1e-3, (losses, losses_ref)
    sd, sd_ref = model.state_dict(), ref.state_dict()
    for name in sd_ref:
        a, b = sd[name].detach().cpu(), sd_ref[name]
        if not a.is_floating_point():
            assert torch.equal(a, b), name
        elif name.endswith("nn.0.bias") or name.endswith("encode_all.0.bias"):
            # a bias in front of a train-mode BatchNorm has an exactly-zero true gradient; what both implementations
            # feed Adam is rounding noise, which Adam normalises to +-lr per step: bounded, not comparable
            assert float((a - b).abs().max()) <= 2 * 8 * 1e-3 * 1.05, name   # each side moves at most lr per step
        elif name.endswith("running_mean"):
            # the BatchNorm right behind such a bias tracks the mean of an input that contains it
            torch.testing.assert_close(a, b, rtol=2e-3, atol=2 * 8 * 1e-3 * 1.05, msg=lambda m, n=name: f"{n}: {m}")
        else:
            torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-4, msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("flow,optimizer", [("dynamic", "torch"), ("static-table", "torch"), ("dynamic", "flat")])
def test_graphed_train_step_matches_eager(dev, flow, optimizer):
    """H1: the step replayed as two hipGraphs (parallel.GraphedTrainStep) walks the same parameter trajectory as the
    eager step (every kernel on the path is deterministic, so the comparison is bitwise) -- for the kNN flow and for
    the reference's active flow with the radius table built inside the captured step (train.py:45-48); with torch's
    capturable AdamW and with optim.FlatAdamW, whose learning rate is changed between replays the way
    ReduceLROnPlateau (train.py:58,76) would."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from deepmetv2_amd.model import Net
    from deepmetv2_amd.optim import FlatAdamW
    from deepmetv2_amd.parallel import FlatModule, GradSync, GraphedTrainStep, train_step
    sizes = [700, 90, 1300]
    x, y, batch, ptr = synth.make_events(sizes, seed=5, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes))

    def radius(xx):
        etaphi = torch.stack([xx[:, 3], torch.atan2(xx[:, 1], xx[:, 0])], 1)
        return dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)

    graph_fn = radius if flow == "static-table" else None
    finals = []
    for graphed in (False, True):
        torch.manual_seed(1)
        model = Net(8, 3, graph="dynamic" if flow == "dynamic" else "static", k=16).to(dev).train()
        flat = FlatModule(model); sync = GradSync(flat)
        if optimizer == "flat":
            opt = FlatAdamW([flat.flat_param], lr=1e-3)
        else:
            opt = torch.optim.AdamW([flat.flat_param], lr=1e-3, capturable=True)
        if graphed:
            p0 = flat.flat_param.detach().clone()
            bufs0 = [b.detach().clone() for b in model.buffers()]
            step = GraphedTrainStep(model, flat, sync, opt, x, y, batch, ptr, warmup=1, graph_fn=graph_fn)
            # capture ran warm-up steps: rewind parameters, buffers and optimizer state
            with torch.no_grad():
                flat.flat_param.copy_(p0)
                for b, b0 in zip(model.buffers(), bufs0):
                    b.copy_(b0)
                for st in opt.state.values():
                    for name, v in st.items():
                        if name == "bias_pow":
                            v.fill_(1.0)          # beta^0
                        elif torch.is_tensor(v) and name != "lr_dev":
                            v.zero_()
        for it in range(4):
            if it == 2 and optimizer == "flat":
                opt.param_groups[0]["lr"] = 2.5e-4     # a scheduler steps between two training steps
            if graphed:
                loss = step()
            else:
                loss = train_step(model, flat, sync, opt, x, y, batch, ptr,
                                  edge_index=graph_fn(x) if graph_fn is not None else None)
        torch.cuda.synchronize()
        finals.append((flat.flat_param.detach().clone(), float(loss)))
    assert finals[0][1] == finals[1][1]
    assert torch.equal(finals[0][0], finals[1][0])


@pytest.mark.parametrize("ncols", [6, 11])
def test_eval_metrics_match_oracle(dev, ncols):
    """N4: `resolution`, `u_perp_par_loss` and the `metrics` registry (reference model/net.py:64-161) against the
    oracle's restatement; the per-event MET sums come from the HIP reduction."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from oracle import ref_ops
    sizes = [500, 3, 1200, 64]
    x, y, batch, ptr = synth.make_events(sizes, seed=8)
    y = y[:, :ncols].contiguous()
    g = torch.Generator().manual_seed(1)
    w = torch.rand(x.shape[0], generator=g).requires_grad_(True)
    res_ref, qt_ref = ref_ops.resolution(w, x, y, batch)
    loss_ref = ref_ops.u_perp_par_loss(w, x, y, batch)
    loss_ref.backward()
    wd = w.detach().to(dev).requires_grad_(True)
    res, qt = dm.metrics["resolution"](wd, x.to(dev), y.to(dev), batch.to(dev))
    loss = dm.u_perp_par_loss(wd, x.to(dev), y.to(dev), batch.to(dev))
    loss.backward()
    assert set(res) == set(res_ref) and (("deepMETResponse" in res) == (ncols > 6))
    scale = float((w.detach().abs() * x[:, :2].abs().sum(1)).sum() / len(sizes))
    for name in res_ref:
        for a, r in zip(res[name], res_ref[name]):
            import numpy as np
            np.testing.assert_allclose(a, r, rtol=1e-4, atol=1e-5 * scale)
    import numpy as np
    np.testing.assert_allclose(qt, qt_ref, rtol=1e-6)
    torch.testing.assert_close(loss.detach().cpu(), loss_ref.detach(), rtol=1e-4, atol=1e-6 * scale * scale)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=1e-3, atol=1e-5 * float(w.grad.abs().max()))


def test_ops_fail_loudly_without_gpu_tensor(dev):
    import deepmetv2_amd as dm
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        dm.knn_graph(torch.randn(10, 4), 2)


@pytest.mark.parametrize("H,H1,H2,k,aggr,act2", [(32, 48, 32, 16, "max", True), (32, 64, 64, 8, "add", True),
                                               (64, 96, 64, 16, "max", True), (64, 128, 64, 32, "add", False),
                                               (32, 33, 32, 16, "max", False)])
def test_edge_mlp2_bf16_mfma(dev, H, H1, H2, k, aggr, act2):
    """BASELINE configs[2] for a GENERIC nn (the DRN call shape, model/dynamic_reduction_network.py:59-63,86-87):
    Linear - ELU - Linear [- ELU] per edge on the bf16 matrix cores, fused with the max / add aggregation
    (csrc/edgemlp.hip).  (a) tight against a torch emulation of the same recipe (inputs, weights and the hidden
    activations rounded to bf16, fp32 accumulation); (b) within the bf16 bar of rule R6 (rtol 2e-2 of the output scale)
    of the fp32 PyG-shaped oracle; (c) gradients -- the backward differentiates the fp32 operators -- against the
    oracle's; the graph is the fp32-exact kNN either way."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    sizes = [300, 5, 0, 131, 64]          # an event smaller than k (empty slots) and an empty event
    x, batch, ptr = _ragged(sizes, H, seed=300 + H1 + k)
    layers = [torch.nn.Linear(2 * H, H1), torch.nn.ELU(), torch.nn.Linear(H1, H2)] + ([torch.nn.ELU()] if act2 else [])
    nn_ = torch.nn.Sequential(*layers)
    conv = dm.DynamicEdgeConv(nn=nn_, k=k, aggr=aggr)
    conv.compute_dtype = torch.bfloat16
    xr = x.clone().requires_grad_(True)
    out_ref = ref_ops.dynamic_edge_conv(xr, batch, nn_, k, aggr)
    gup = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(2))
    out_ref.backward(gup)
    g_ref = [xr.grad.clone()] + [p.grad.clone() for p in nn_.parameters()]
    nn_.zero_grad()
    # torch emulation of the bf16 recipe on the oracle's graph
    nbr_ref, _ = ref_ops.knn_table(x, ptr, k)
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    l1, l2 = nn_[0], nn_[2]
    j = nbr_ref.long().clamp(min=0)
    xi = x.unsqueeze(1).expand(-1, k, -1)
    feat = torch.cat([bf(xi), bf(x[j] - xi)], -1)
    h1 = bf(torch.nn.functional.elu(feat @ bf(l1.weight.detach()).T + l1.bias.detach()))
    m = h1 @ bf(l2.weight.detach()).T + l2.bias.detach()
    if act2:
        m = torch.nn.functional.elu(m)
    ok = (nbr_ref >= 0).unsqueeze(-1)
    if aggr == "max":
        emu = torch.where(ok, m, torch.full_like(m, float("-inf"))).max(1).values
        emu = torch.where(torch.isinf(emu), torch.zeros_like(emu), emu)
    else:
        emu = torch.where(ok, m, torch.zeros_like(m)).sum(1)

    conv = conv.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, batch.to(dev))
    out.backward(gup.to(dev))
    o = out.detach().cpu()
    scale = float(out_ref.detach().abs().max())
    torch.testing.assert_close(o, emu, rtol=2e-3, atol=2e-3 * scale)                        # (a)
    torch.testing.assert_close(o, out_ref.detach(), rtol=2e-2, atol=2e-2 * scale)           # (b)
    got = [xd.grad.cpu()] + [p.grad.cpu() for p in nn_.parameters()]
    for g, gr in zip(got, g_ref):                                                           # (c)
        torch.testing.assert_close(g, gr, rtol=2e-3, atol=2e-4 * max(float(gr.abs().max()), 1e-6))


@pytest.mark.parametrize("H,H1,H2,k,aggr,negative_gamma", [(32, 48, 32, 16, "add", False), (32, 64, 64, 8, "max", True),
                                                           (64, 96, 64, 16, "add", True), (64, 96, 64, 16, "max", False)])
def test_edge_mlp2_bf16_with_trailing_batch_norm(dev, H, H1, H2, k, aggr, negative_gamma):
    """The DRN's edge MLP as written (model/dynamic_reduction_network.py:59-70: Linear - ELU - Linear - ELU - BatchNorm1d
    over the MESSAGES, aggr add by default): fused on the bf16 matrix cores, the norm applied after the aggregation by
    the affine-commutes argument (max: the minimum where gamma < 0).  Training mode against the fp32 PyG-shaped oracle
    with the same module: output at the bf16 bar, running statistics and num_batches_tracked moved exactly once per
    forward + backward, gradients (the backward differentiates the fp32 operators) against the oracle's; then eval mode
    (running statistics) against the oracle in eval mode."""
    import copy
    import deepmetv2_amd as dm
    from oracle import ref_ops
    sizes = [300, 5, 0, 131, 64]
    x, batch, ptr = _ragged(sizes, H, seed=500 + H1 + k)
    bn = torch.nn.BatchNorm1d(H2)
    nn_ = torch.nn.Sequential(torch.nn.Linear(2 * H, H1), torch.nn.ELU(), torch.nn.Linear(H1, H2), torch.nn.ELU(), bn)
    conv = dm.DynamicEdgeConv(nn=nn_, k=k, aggr=aggr)      # (the constructor re-initialises nn, like upstream's)
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(-1.5, 1.5, H2) if negative_gamma else torch.linspace(0.5, 1.5, H2))
        bn.bias.copy_(torch.linspace(-0.3, 0.3, H2))
    ref_nn = copy.deepcopy(nn_)
    xr = x.clone().requires_grad_(True)
    out_ref = ref_ops.dynamic_edge_conv(xr, batch, ref_nn, k, aggr)
    gup = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(3))
    out_ref.backward(gup)
    g_ref = [xr.grad.clone()] + [p.grad.clone() for p in ref_nn.parameters()]
    conv = conv.to(dev)
    conv.compute_dtype = torch.bfloat16
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, batch.to(dev))
    out.backward(gup.to(dev))
    scale = float(out_ref.detach().abs().max())
    torch.testing.assert_close(out.detach().cpu(), out_ref.detach(), rtol=3e-2, atol=3e-2 * scale)
    assert int(bn.num_batches_tracked) == int(ref_nn[4].num_batches_tracked) == 1
    torch.testing.assert_close(bn.running_mean.cpu(), ref_nn[4].running_mean, rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(bn.running_var.cpu(), ref_nn[4].running_var, rtol=3e-2, atol=2e-3)
    got = [xd.grad.cpu()] + [p.grad.cpu() for p in nn_.parameters()]
    for g, gr in zip(got, g_ref):
        torch.testing.assert_close(g, gr, rtol=2e-3, atol=3e-4 * max(float(gr.abs().max()), 1e-6))
    # eval mode: running statistics (make both sides use the oracle's so that only the kernel differs)
    with torch.no_grad():
        bn.running_mean.copy_(ref_nn[4].running_mean.to(dev)); bn.running_var.copy_(ref_nn[4].running_var.to(dev))
    conv.eval(); ref_nn.eval()
    with torch.no_grad():
        o_eval = conv(x.to(dev), batch.to(dev)).cpu()
        o_eval_ref = ref_ops.dynamic_edge_conv(x, batch, ref_nn, k, aggr)
    torch.testing.assert_close(o_eval, o_eval_ref, rtol=3e-2, atol=3e-2 * float(o_eval_ref.abs().max()))
    assert int(bn.num_batches_tracked) == 1


def test_counted_gather_winner_ids_and_ordered_rows(dev):
    """N1 / the reference's active flow (train.py:48: one 255-wide radius table per batch): the winner-id form of the
    counted LDS gather (rows walked in order of their depth) must give the slot form's output bit for bit, its ids must
    be the slot form's winners, and the backward scatter fed by the ids must equal the one that looks the ids up."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    _default_path_only("DMET_GATHER_MAX_FORM", "l2-only", "the winner-id form is an LDS-resident kernel reading slice-major tables")
    g = torch.Generator().manual_seed(31)
    sizes = [1200, 0, 37, 900, 2100]
    N = sum(sizes)
    etaphi = torch.stack([(torch.rand(N, generator=g) - 0.5) * 5, (torch.rand(N, generator=g) - 0.5) * 6.28], 1)
    etaphi[100:400] = etaphi[100] + 0.05 * torch.randn(300, 2, generator=g)       # rows that overflow the 255 slots
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    t = dm.radius_table(etaphi.to(dev), 0.4, batch, loop=True, max_num_neighbors=255)
    assert t.nonempty and int(t.cnt.min()) >= 1 and int(t.cnt.max()) == 255
    H = 32
    x = torch.randn(N, H, generator=g).to(dev)
    W = (torch.randn(H, 2 * H, generator=g) / 8).to(dev)
    b = torch.randn(H, generator=g).to(dev)
    order = t.order_by_count()
    lo = torch.repeat_interleave(t.ptr[:-1], t.ptr.diff()).view(-1, 1)
    for b_ in range(len(sizes)):           # a permutation of every event, deepest rows first
        s, e = int(t.ptr[b_]), int(t.ptr[b_ + 1])
        o = order[s:e].long()
        assert sorted(o.tolist()) == list(range(e - s))
        c = t.cnt[s:e][o]
        assert bool((c[1:] <= c[:-1]).all())
    for sliced in (False, True):
        P, Q = _native.node_linear_split(x, W, b, sliced=sliced)
        out0, arg8 = _native.gather_max(P, Q, t.nbr, t.ptr, want_arg=True, cnt=t.cnt, lds=True, sliced=sliced)
        out1, argj = _native.gather_max_counted_j16(P, Q, t.nbr, t.cnt, order, t.ptr, sliced)
        assert torch.equal(out0, out1)
        win = torch.gather(t.nbr.long(), 1, arg8.long()) - lo
        assert torch.equal(argj.long() & 0xFFFF, win)
        out2, argj2 = _native.gather_max_counted_j16(P, Q, t.nbr, t.cnt, None, t.ptr, sliced)      # without the order
        assert torch.equal(out1, out2) and torch.equal(argj, argj2)
        # ids from the uint16 rows written by the radius kernel: same bits again
        if _native.RADIUS_FORM != "sweep":     # the all-pairs form (DMET_RADIUS=sweep) writes the int32 table only
            assert t.rows16 is not None and t.rows16.shape == (N, 256)
            out4, argj4 = _native.gather_max_local_j16(P, Q, t.rows16, t.cnt, order, t.ptr, t.k, sliced)
            assert torch.equal(out1, out4) and torch.equal(argj, argj4)
    # the uint16 rows themselves: slots < cnt = local ids, the rest of the last started chunk = 0xFFFF
    if t.rows16 is not None:
        slot = torch.arange(256, device=dev).view(1, -1)
        c = t.cnt.long().view(-1, 1)
        r16 = t.rows16.long() & 0xFFFF
        want = torch.zeros_like(r16); want[:, :255] = t.nbr.long() - lo
        assert torch.equal(torch.where(slot < c, r16, 0 * r16), torch.where(slot < c, want, 0 * want))
        pad = (slot >= c) & (slot < (c + 7) // 8 * 8)
        assert bool((r16[pad] == 0xFFFF).all())
    gout = torch.randn(N, H, generator=g).to(dev)
    gq0 = _native.gather_max_bwd_lds(gout, arg8, t.nbr, t.ptr)
    gq1 = _native.gather_max_bwd_j16(gout, argj, t.ptr)
    assert torch.equal(gq0, gq1)           # integer LDS sums: bitwise, whatever the order of the atomics


@pytest.mark.parametrize("sizes,k,sliced", [([4500, 4500, 300, 2100], 16, True), ([4500, 77, 0, 2500], 16, False),
                                             ([50, 450, 800], 16, True), ([3000, 1], 8, True), ([2200, 2300], 20, False)])
def test_knn_build_carries_the_dense_layer(dev, sizes, k, sliced):
    """dmet_knn_local_dense_f32: the node-level dense layer computed by trailing workgroups of the filter launch has the
    bits of dmet_node_linear_split_(sliced_)f32, and the graph is the one of dmet_knn_local_f32 (= the oracle's)."""
    from deepmetv2_amd import _native
    from oracle import ref_ops
    x, batch, ptr = _ragged(sizes, 32, 77)
    g = torch.Generator().manual_seed(5)
    W = torch.randn(32, 64, generator=g) * 0.2
    b = torch.randn(32, generator=g)
    xd, pd, Wd, bd = x.to(dev), ptr.to(dev), W.to(dev), b.to(dev)
    for bias in (bd, None):
        nbr, dist, loc, pq = _native.knn_local_dense(xd, pd, k, Wd, bias, sliced)
        if pq is None:   # diagnostic switches that take the build off the second filter form (tools/toggle_sweep.sh)
            import os
            assert os.environ.get("DMET_KNN_PATH") or os.environ.get("DMET_KNN_FILTER"), \
                "a 32-feature build with k <= 20 takes the matrix-core path and carries the dense layer"
            pytest.skip("this build cannot carry the dense layer (diagnostic switch)")
        P_ref, Q_ref = _native.node_linear_split(xd, Wd, bias, sliced=sliced)
        assert pq[2] == sliced and torch.equal(pq[0], P_ref) and torch.equal(pq[1], Q_ref)
        nbr0, dist0, loc0 = _native.knn_local(xd, pd, k)
        assert torch.equal(nbr, nbr0) and torch.equal(dist, dist0) and torch.equal(loc, loc0)
    nbr_ref, _ = ref_ops.knn_table(x, ptr, k)
    assert torch.equal(nbr.cpu(), nbr_ref)
    # layout 2 (BASELINE configs[2]): bf16 operands, Q stored as bf16 -- the bits of dmet_node_linear_split_bf16
    nbr, dist, loc, pq = _native.knn_local_dense(xd, pd, k, Wd, bd, "bf16")
    P_ref, Qh_ref = _native.node_linear_split_bf16(xd, Wd, bd)
    assert pq is not None and pq[2] == "bf16" and pq[1].dtype == torch.bfloat16
    assert torch.equal(pq[0], P_ref) and torch.equal(pq[1].view(torch.int16), Qh_ref.view(torch.int16))
    assert torch.equal(nbr.cpu(), nbr_ref)


def test_knn_build_without_matrix_core_path_leaves_the_dense_layer(dev, monkeypatch):
    """Builds that cannot carry the dense layer say so (pq None) and DynamicEdgeConv launches it itself: same output."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, conv
    x, batch, ptr = _ragged([300, 500], 32, 3)
    xd, pd = x.to(dev), ptr.to(dev)
    W = torch.randn(32, 64, device=dev)
    assert _native.knn_local_dense(xd, pd, 32, W, None, False)[3] is None        # k > 20: exact kernel
    x16 = torch.randn(800, 16, device=dev)
    assert _native._knn(x16, pd, 16, None, True, dense=(W, None, False))[3] is None   # 16 features
    torch.manual_seed(0)
    layer = dm.DynamicEdgeConv(torch.nn.Linear(64, 32), k=16).to(dev)
    out1 = layer(xd, batch.to(dev))
    monkeypatch.setattr(conv, "KNN_RIDER", "0")
    out0 = layer(xd, batch.to(dev))
    assert torch.equal(out0, out1)


@pytest.mark.parametrize("wd", [1e-2, 0.0])
def test_flat_adamw_matches_torch_adamw(dev, wd):
    """dmet_adamw_f32 (train.py:75's optimizer on the flat parameter tensor) against torch.optim.AdamW, 25 steps."""
    from deepmetv2_amd.optim import FlatAdamW
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(6641, generator=g)
    pa = torch.nn.Parameter(p0.clone().to(dev))
    pb = torch.nn.Parameter(p0.clone().double())           # fp64 torch reference on the CPU
    oa = FlatAdamW([pa], lr=1e-3, weight_decay=wd)
    ob = torch.optim.AdamW([pb], lr=1e-3, weight_decay=wd)
    for it in range(25):
        gr = torch.randn(6641, generator=g) * (10.0 ** ((it % 5) - 3))
        pa.grad = gr.to(dev)
        pb.grad = gr.double()
        oa.step()
        ob.step()
    st = oa.state[pa]
    assert float(st["step"]) == 25.0
    torch.testing.assert_close(pa.detach().cpu().double(), pb.detach(), rtol=2e-6, atol=2e-7)
    # the moments are sums of terms of either sign and of magnitudes 1e-3 .. 10: fp32 rounding relative to the largest
    m_ref, v_ref = ob.state[pb]["exp_avg"], ob.state[pb]["exp_avg_sq"]
    torch.testing.assert_close(st["exp_avg"].cpu().double(), m_ref, rtol=1e-5, atol=1e-6 * float(m_ref.abs().max()))
    torch.testing.assert_close(st["exp_avg_sq"].cpu().double(), v_ref, rtol=1e-5, atol=1e-6 * float(v_ref.abs().max()))


def test_flat_adamw_continues_a_torch_adamw_state(dev):
    """A checkpoint written with torch.optim.AdamW (utils.py:59-77 saves `optim_dict`; state keys step / exp_avg /
    exp_avg_sq only) loads into FlatAdamW: beta^step and the device learning rate are rebuilt, the run continues on the
    trajectory of the fp64 reference; FlatAdamW's own state_dict round-trips too."""
    import copy
    from deepmetv2_amd.optim import FlatAdamW
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(6641, generator=g)
    pt = torch.nn.Parameter(p0.clone().to(dev))
    pb = torch.nn.Parameter(p0.clone().double())
    ot = torch.optim.AdamW([pt], lr=1e-3)
    ob = torch.optim.AdamW([pb], lr=1e-3)
    grads = [torch.randn(6641, generator=g) * (10.0 ** ((it % 4) - 2)) for it in range(14)]
    for it in range(5):
        pt.grad = grads[it].to(dev); pb.grad = grads[it].double()
        ot.step(); ob.step()
    pa = torch.nn.Parameter(pt.detach().clone())
    oa = FlatAdamW([pa], lr=1e-3)
    oa.load_state_dict(copy.deepcopy(ot.state_dict()))     # (as from a file: load_state_dict itself keeps references)
    for it in range(5, 10):
        pa.grad = grads[it].to(dev); pb.grad = grads[it].double()
        oa.step(); ob.step()
    assert float(oa.state[pa]["step"]) == 10.0
    torch.testing.assert_close(pa.detach().cpu().double(), pb.detach(), rtol=2e-6, atol=4e-7)
    # round trip of its own state (load_state_dict casts the double state tensors to fp32: they are rebuilt)
    pc = torch.nn.Parameter(pa.detach().clone())
    oc = FlatAdamW([pc], lr=1e-3)
    oc.load_state_dict(copy.deepcopy(oa.state_dict()))
    for it in range(10, 14):
        pa.grad = grads[it].to(dev); pc.grad = grads[it].to(dev); pb.grad = grads[it].double()
        oa.step(); oc.step(); ob.step()
    torch.testing.assert_close(pc.detach().cpu().double(), pb.detach(), rtol=2e-6, atol=6e-7)
    torch.testing.assert_close(pc.detach(), pa.detach(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("sizes,with_res", [([4500, 4500, 300, 2100], True), ([50, 450, 800, 0, 3], True), ([3000, 77], False)])
def test_batch_norm_transform_rides_in_the_knn_prep(dev, sizes, with_res):
    """dmet_bn_knn_local_dense_f32: y = residual + BN(raw) written by the build's prep launch has the bits of dmet_bn_fwd_f32,
    and graph / dense layer are those of a build on that y."""
    from deepmetv2_amd import _native
    x, batch, ptr = _ragged(sizes, 32, 21)
    g = torch.Generator().manual_seed(9)
    res = torch.randn(x.shape, generator=g) if with_res else None
    gamma, beta = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    W, b = torch.randn(32, 64, generator=g) * 0.2, torch.randn(32, generator=g)
    xd, pd = x.to(dev), ptr.to(dev)
    rd = res.to(dev) if with_res else None
    gd, bd, Wd, bbd = gamma.to(dev), beta.to(dev), W.to(dev), b.to(dev)
    rm, rv = torch.zeros(32, device=dev), torch.ones(32, device=dev)
    y_ref, mean_ref, inv_ref = _native.bn_fwd(xd, rd, gd, bd, 1e-5, 0.1, rm.clone(), rv.clone(), True)
    rm2, rv2 = rm.clone(), rv.clone()
    mean, invstd = _native.bn_stats(xd, 1e-5, 0.1, rm2, rv2)
    assert torch.equal(mean, mean_ref) and torch.equal(invstd, inv_ref)
    out = _native.bn_knn_local_dense(xd, rd, gd, bd, mean, invstd, pd, 16, (Wd, bbd, True))
    import os
    if os.environ.get("DMET_KNN_PATH") == "exact":
        # documented property, not a silenced failure: the exact kernel has no prep launch for the transform to ride in,
        # dmet_bn_knn_local_dense_f32 then launches NOTHING (*fused = 0, _native returns None) and dense.batch_norm takes
        # the separate pass -- whose bits are the reference of this test anyway; the build on its output must agree
        assert out is None
        nbr0, dist0, loc0 = _native.knn_local(y_ref, pd, 16)
        nbr_ref, dist_ref = __import__("oracle.ref_ops", fromlist=["x"]).knn_table(y_ref.cpu(), ptr, 16)
        assert torch.equal(nbr0.cpu(), nbr_ref) and torch.equal(dist0.cpu(), dist_ref)
        return
    # (DMET_KNN_FILTER=1, the first filter form for every event, shares the prep launch: the test runs unchanged)
    assert out is not None, "a 32-feature build with k <= 20 takes the matrix-core path"
    y, nbr, dist, loc, pq = out
    assert torch.equal(y, y_ref)
    nbr0, dist0, loc0, pq0 = _native.knn_local_dense(y_ref, pd, 16, Wd, bbd, True)
    assert torch.equal(nbr, nbr0) and torch.equal(dist, dist0) and torch.equal(loc, loc0)
    if os.environ.get("DMET_KNN_FILTER") == "1":
        # the first filter form alone (knn_filter_kernel, every event) carries the BatchNorm transform in the shared prep
        # launch (everything above held) but has no rider workgroups for the dense layer: both entries report
        # dense_done = 0 and the layer launches node_linear_split itself (conv._EdgeConvLinearMax)
        assert pq is None and pq0 is None
        return
    assert pq is not None and torch.equal(pq[0], pq0[0]) and torch.equal(pq[1], pq0[1])


def test_model_with_fused_transform_matches_unfused(dev, monkeypatch):
    """The whole model, forward and backward, with the BatchNorm transforms inside the graph builds / the head's forward
    launch and without."""
    from deepmetv2_amd import conv, dense, synth
    from deepmetv2_amd.model import Net, loss_fn, split_features
    x, y, batch, ptr = synth.make_events([900, 2500, 64, 300], seed=4)
    xd, yd, bd = x.to(dev), y.to(dev), batch.to(dev)
    torch.manual_seed(1)
    model = Net(8, 3, graph="dynamic", k=16).to(dev).train()
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setattr(conv, "BN_KNN_FUSE", fuse)
        monkeypatch.setattr(dense, "HEAD_FUSE", fuse)      # the last block's transform inside the head's forward launch
        monkeypatch.setattr(dense, "ENC_BN_FUSE", fuse)    # bn_all's backward transform inside the encoder's backward kernel
        for bn in [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]:
            bn.reset_running_stats()
        model.zero_grad(set_to_none=True)
        xc, xk = split_features(xd)
        w = model(xc, xk, None, bd)
        loss = loss_fn(w, xd, yd, bd)
        loss.backward()
        outs.append((w.detach().clone(), [p.grad.clone() for p in model.parameters()],
                     [b.clone() for b in model.buffers()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a, b)
    # eval mode (evaluate.py): the transforms use the running statistics, fused or not
    model.eval()
    ev = []
    with torch.no_grad():
        for fuse in ("1", "0"):
            monkeypatch.setattr(conv, "BN_KNN_FUSE", fuse)
            monkeypatch.setattr(dense, "HEAD_FUSE", fuse)
            ev.append(model(*split_features(xd), None, bd).clone())
    assert torch.equal(ev[0], ev[1])


def test_async_graph_build_matches_inline(dev):
    """graph.build_async: the radius table built on a side stream beside the encoder and joined by the first EdgeConv gives
    the bits of the inline build -- eager and inside a captured step (parallel.GraphedTrainStep)."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from deepmetv2_amd.model import Net
    from deepmetv2_amd.optim import FlatAdamW
    from deepmetv2_amd.parallel import FlatModule, GradSync, GraphedTrainStep, train_step
    sizes = [700, 90, 1300]
    x, y, batch, ptr = synth.make_events(sizes, seed=15, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))

    def radius(xx):
        etaphi = torch.stack([xx[:, 3], torch.atan2(xx[:, 1], xx[:, 0])], 1)
        return dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)

    finals = []
    for mode in ("inline", "async", "async-graphed"):
        torch.manual_seed(4)
        model = Net(8, 3, graph="static", k=16).to(dev).train()
        flat = FlatModule(model); sync = GradSync(flat)
        opt = FlatAdamW([flat.flat_param], lr=1e-3)
        graph_fn = radius if mode == "inline" else (lambda xx: dm.build_async(lambda: radius(xx)))
        if mode == "async-graphed":
            p0 = flat.flat_param.detach().clone()
            bufs0 = [b.detach().clone() for b in model.buffers()]
            step = GraphedTrainStep(model, flat, sync, opt, x, y, batch, ptr, warmup=1, graph_fn=graph_fn)
            with torch.no_grad():
                flat.flat_param.copy_(p0)
                for b, b0 in zip(model.buffers(), bufs0):
                    b.copy_(b0)
                for st in opt.state.values():
                    for name, v in st.items():
                        if name == "bias_pow":
                            v.fill_(1.0)
                        elif torch.is_tensor(v) and name != "lr_dev":
                            v.zero_()
        for _ in range(3):
            loss = step() if mode == "async-graphed" else train_step(model, flat, sync, opt, x, y, batch, ptr,
                                                                     edge_index=graph_fn(x))
        torch.cuda.synchronize()
        finals.append((flat.flat_param.detach().clone(), float(loss)))
    for other in finals[1:]:
        assert other[1] == finals[0][1] and torch.equal(other[0], finals[0][0])


@pytest.mark.parametrize("graph_kind", ["table", "edge_index", "future"])
def test_static_model_with_transform_in_the_dense_layer_matches_unfused(dev, monkeypatch, graph_kind):
    """The reference's active flow (one radius graph per batch, model/graph_met_network.py:65): the BatchNorm transform that
    produces an EdgeConv's input formed inside that layer's node-level dense layer launch (dmet_bn_node_linear_split_f32,
    EdgeConv.prebuild_hook) against the separate transform pass -- whole model, forward, backward, buffers, bit for bit;
    with the graph handed over as the table, as radius_graph's [2,E] tensor and as a side-stream future; an event beyond
    the LDS image (row-major P / Q) included; eval mode too."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, synth
    from deepmetv2_amd.model import Net, loss_fn, split_features
    sizes = [900, 2500, 64, 5300] if graph_kind == "table" else [900, 2500, 64, 300]
    x, y, batch, ptr = synth.make_events(sizes, seed=14, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    etaphi = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1)

    def graph():
        if graph_kind == "edge_index":
            return dm.radius_graph(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)
        build = lambda: dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)
        return dm.build_async(build) if graph_kind == "future" else build()

    torch.manual_seed(6)
    model = Net(8, 3, graph="static", k=16).to(dev).train()
    calls = []
    real = _native.bn_node_linear_split

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(_native, "bn_node_linear_split", spy)
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DMET_BN_NLS_FUSE", fuse)
        for bn in [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]:
            bn.reset_running_stats()
        model.zero_grad(set_to_none=True)
        n0 = len(calls)
        w = model(*split_features(x), graph(), batch)
        loss = loss_fn(w, x, y, batch)
        loss.backward()
        # both EdgeConv layers take their input that way on the default path; under DMET_EDGECONV_FORM=fused no layer
        # has a separate dense-layer launch to carry it, under DMET_FUSED_ENCODER=0 the first layer's input comes from the
        # layer-by-layer encoder route, which has no hook (tools/toggle_sweep.sh)
        from deepmetv2_amd import conv as conv_mod
        expect = 0 if (fuse == "0" or conv_mod.EDGECONV_FORM != "split") else (2 if model.graphnet.fused_encoder else 1)
        assert len(calls) - n0 == expect
        outs.append((w.detach().clone(), [p.grad.clone() for p in model.parameters()], [b.clone() for b in model.buffers()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a, b)
    model.eval()
    ev = []
    with torch.no_grad():
        for fuse in ("1", "0"):
            monkeypatch.setenv("DMET_BN_NLS_FUSE", fuse)
            ev.append(model(*split_features(x), graph(), batch).clone())
    assert torch.equal(ev[0], ev[1])


def test_deferred_weight_gradient_sums_same_bits(dev, monkeypatch):
    """K5 / N3 (train.py:51-52): with the weight-gradient sums of the EdgeConv dense layers, the encoder and the head left
    to ONE launch at the end of the backward pass (dmet_finalize_defer_begin / dmet_finalize_flush, what train_step does)
    every parameter gradient, the loss and the updated parameters carry the bits of the per-call sums -- and four calls
    were really queued."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _lib, _native, synth
    from deepmetv2_amd.model import Net
    from deepmetv2_amd.optim import FlatAdamW
    from deepmetv2_amd.parallel import FlatModule, GradSync, train_step
    sizes = [900, 70, 1300, 33]
    x, y, batch, ptr = synth.make_events(sizes, seed=11, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    queued = []
    real_flush = _native.finalize_flush

    def counting_flush():
        queued.append(_lib.load().dmet_finalize_pending())
        real_flush()

    monkeypatch.setattr(_native, "finalize_flush", counting_flush)
    results = []
    for defer in (False, True):
        monkeypatch.setattr(_native, "DEFER_FINALIZE", defer)
        torch.manual_seed(3)
        model = Net(8, 3, graph="dynamic", k=16).to(dev).train()
        flat = FlatModule(model); sync = GradSync(flat)
        opt = FlatAdamW([flat.flat_param], lr=1e-3)
        losses = [float(train_step(model, flat, sync, opt, x, y, batch, ptr)) for _ in range(3)]
        results.append((losses, flat.flat_grad.detach().clone(), flat.flat_param.detach().clone()))
    (l0, g0, p0), (l1, g1, p1) = results
    assert l0 == l1 and torch.equal(g0, g1) and torch.equal(p0, p1)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    # two EdgeConv layers, the encoder, the head (the layer-by-layer routes of DMET_FUSED_ENCODER=0 have no partials of
    # their own to queue); nothing queued without the deferral
    n = 2 if os.environ.get("DMET_FUSED_ENCODER", "1") == "0" else 4
    assert queued == [-1, -1, -1, n, n, n]
    assert _lib.load().dmet_finalize_pending() == -1


def test_knn_size_hint_right_and_wrong(dev):
    """K1: dmet_knn_size_hint drops the merge launch of the first filter form's tail items when the caller says every event
    takes the second form.  A RIGHT hint changes no bit; a WRONG one (small events present after all) costs time only:
    their tail queries go through the exact kernel and the table still equals the oracle's."""
    from deepmetv2_amd import _native
    from oracle import ref_ops
    k = 16
    # (a) every event >= 800 nodes
    x, _b, ptr = _ragged([900, 1500, 810], 32, seed=41)
    ref = ref_ops.knn_table(x, ptr, k)
    _native.knn_size_hint(810, 1500)
    nbr, dist, st = _knn_with_stats(x.to(dev), ptr.to(dev), k)
    assert torch.equal(nbr, ref[0]) and torch.equal(dist, ref[1]) and st["flagged_queries"] == 0
    # the hint is spent: the next build (first-form events) is an ordinary one
    x2, _b2, ptr2 = _ragged([300, 120, 500], 32, seed=42)
    ref2 = ref_ops.knn_table(x2, ptr2, k)
    nbr2, dist2, st2 = _knn_with_stats(x2.to(dev), ptr2.to(dev), k)
    assert torch.equal(nbr2, ref2[0]) and torch.equal(dist2, ref2[1]) and st2["flagged_queries"] == 0
    # (b) a hint that rules out events that are there: 12 first-form events in the split tail of a batch of 30 x 4500
    # (2 130 whole-sweep tiles + 120 tiles of the small events: more than the 2 048 wavefront slots)
    sizes = [4500] * 30 + [600] * 12
    x3, _b3, ptr3 = _ragged(sizes, 32, seed=43)
    xd, pd = x3.to(dev), ptr3.to(dev)
    nbr_a, dist_a, st_a = _knn_with_stats(xd, pd, k)
    assert st_a["flagged_queries"] == 0
    _native.knn_size_hint(800, 4500)
    nbr_b, dist_b, st_b = _knn_with_stats(xd, pd, k)
    assert torch.equal(nbr_a, nbr_b) and torch.equal(dist_a, dist_b)
    lo = 30 * 4500
    ref3 = ref_ops.knn_table(x3[lo:], ptr3[30:] - lo, k)         # the small events against the oracle
    assert torch.equal(nbr_b[lo:] - lo, ref3[0]) and torch.equal(dist_b[lo:], ref3[1])
    if os.environ.get("DMET_KNN_PATH") != "exact" and os.environ.get("DMET_KNN_FILTER") not in ("0", "1"):   # (1: first form only, the merge launch stays)
        assert st_b["flagged_queries"] > 0   # the tail items of the small events took the exact path instead of the merge


@pytest.mark.parametrize("sizes", [[700, 90, 1300], [4700, 300], [9300, 40]])
def test_backward_scatter_slice_major_handover(dev, sizes):
    """K5: gQ handed from the LDS scatter to the node-level backward kernel slice-major ([8, N, 4]: a scatter workgroup
    writes one contiguous run) carries the bits of the row-major hand-over -- gQ itself (re-laid out) and gx / gW / gb of
    dmet_edgeconv_linear_bwd_sliced_f32 -- for both winner encodings and all three window forms of the scatter (events up
    to 4 608 nodes, up to 9 216, beyond)."""
    from deepmetv2_amd import _native
    H, k = 32, 16
    x, _b, ptr = _ragged(sizes, H, seed=77)
    xd, pd = x.to(dev), ptr.to(dev)
    N = xd.shape[0]
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(32, 64, generator=g) / 8).to(dev)
    g_out = torch.randn(N, H, generator=g).to(dev)
    g_add = torch.randn(N, H, generator=g).to(dev)
    nbr, _d, loc = _native.knn_local(xd, pd, k)
    arg = torch.randint(0, k, (N, H), generator=g, dtype=torch.uint8).to(dev)
    arg[::7, 3] = 255
    # winner ids (uint16 in an int16 tensor) consistent with the slots
    lo = torch.repeat_interleave(pd[:-1], (pd[1:] - pd[:-1])).view(-1, 1)
    win = torch.gather(nbr.long(), 1, arg.long().clamp(max=k - 1)) - lo
    argj = torch.where(arg == 255, torch.full_like(win, 0xFFFF), win).to(torch.int32).to(torch.int16)
    for form in ("slots", "ids"):
        if form == "slots":
            a0 = _native.gather_max_bwd_lds(g_out, arg, nbr, pd, nbr_local=loc, max_nodes=max(sizes))
            a1 = _native.gather_max_bwd_lds(g_out, arg, nbr, pd, nbr_local=loc, max_nodes=max(sizes), sliced=True)
            argk = arg
        else:
            a0 = _native.gather_max_bwd_j16(g_out, argj, pd, max_nodes=max(sizes))
            a1 = _native.gather_max_bwd_j16(g_out, argj, pd, max_nodes=max(sizes), sliced=True)
            argk = argj
        assert tuple(a1.shape) == (8, N, 4)
        assert torch.equal(a1.permute(1, 0, 2).reshape(N, H), a0)
        r0 = _native.edgeconv_linear_bwd(xd, W, g_out, argk, a0, g_add=g_add)
        r1 = _native.edgeconv_linear_bwd(xd, W, g_out, argk, a1, g_add=g_add, gq_sliced=True)
        for u, v in zip(r0, r1):
            assert torch.equal(u, v)


def test_radius_table_without_int32_rows(dev):
    """N1 (train.py:48): with the batch's largest event registered, radius_table writes the event-local uint16 rows only
    (the 255-wide int32 table is not even allocated); the fused EdgeConv -- training AND inference -- reads those, and
    `.nbr`, expanded on demand, equals the table of the int32-writing build slot for slot (first cnt[i] slots, -1 beyond)."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    sizes = [700, 90, 1300, 1, 40]
    x, y, batch, ptr = synth.make_events(sizes, seed=21, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    etaphi = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1).contiguous()
    lazy = dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)
    full = dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255, int32_rows=True)
    if os.environ.get("DMET_RADIUS", "windowed") == "windowed" and os.environ.get("DMET_RADIUS_INT32", "lazy") == "lazy":
        assert not lazy.has_int32_table() and full.has_int32_table()
    assert torch.equal(lazy.cnt, full.cnt)
    conv = dm.EdgeConv(torch.nn.Sequential(torch.nn.Linear(64, 32))).to(dev)
    h = torch.randn(sum(sizes), 32, device=dev)
    outs = {}
    for name, table in (("lazy", lazy), ("full", full)):
        hh = h.clone().requires_grad_(True)
        o = conv(hh, table)
        o.square().sum().backward()
        with torch.no_grad():
            o_eval = conv(h, table)
        outs[name] = (o.detach(), hh.grad.clone(), o_eval, [p.grad.clone() for p in conv.parameters()])
        conv.zero_grad()
    for u, v in zip(outs["lazy"][:3], outs["full"][:3]):
        assert torch.equal(u, v)
    for u, v in zip(outs["lazy"][3], outs["full"][3]):
        assert torch.equal(u, v)
    assert torch.equal(outs["lazy"][0], outs["lazy"][2])       # training and inference forms agree
    default_ids = os.environ.get("DMET_RADIUS_J16", "1") != "0" and os.environ.get("DMET_RADIUS_IDS", "rows16") == "rows16"
    if (os.environ.get("DMET_RADIUS", "windowed") == "windowed" and os.environ.get("DMET_RADIUS_INT32", "lazy") == "lazy"
            and default_ids and os.environ.get("DMET_GATHER_MAX_FORM", "auto") == "auto"):
        assert not lazy.has_int32_table()                       # nobody needed it (the switches above read the int32 rows)
    k = lazy.k
    slot = torch.arange(k, device=dev).view(1, -1)
    used = slot < full.cnt.view(-1, 1)                          # slots beyond cnt[i] are unwritten in a table the build wrote
    minus = torch.full_like(full.nbr, -1)
    assert torch.equal(torch.where(used, lazy.nbr, minus), torch.where(used, full.nbr, minus))
    if os.environ.get("DMET_RADIUS", "windowed") == "windowed" and os.environ.get("DMET_RADIUS_INT32", "lazy") == "lazy" and default_ids:
        assert bool((torch.where(used, minus, lazy.nbr) == -1).all())   # an EXPANDED table is -1 beyond cnt[i]
    assert torch.equal(lazy.edge_index("source_to_target"), full.edge_index("source_to_target"))


def test_deferral_is_not_dropped_by_a_second_begin(dev):
    """K5: beginning a deferral while sums of an earlier one are queued would leave those gradients unwritten for good --
    the C entry refuses, the Python wrapper forms the open deferral's sums first."""
    _default_path_only("DMET_DEFER_FINALIZE", "0", "the deferral is switched off: there is nothing to queue")
    from deepmetv2_amd import _lib, _native
    L = _lib.load()
    N = 700
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(N, 32, generator=g).to(dev)
    params = [(torch.randn(16, 32, generator=g) / 6).to(dev), torch.randn(16, generator=g).to(dev),
              (torch.randn(1, 16, generator=g) / 4).to(dev), torch.randn(1, generator=g).to(dev)]
    out = _native.head_fwd(emb, params)
    g_out = torch.randn(N, generator=g).to(dev)
    want = _native.head_bwd(emb, params, out, g_out)             # sums formed at once
    assert _native.finalize_defer_begin()
    got = _native.head_bwd(emb, params, out, g_out)              # queued
    assert L.dmet_finalize_pending() == 1
    assert L.dmet_finalize_defer_begin() != 0 and b"still queued" in L.dmet_last_error()
    assert _native.finalize_defer_begin()                        # the wrapper flushes the open deferral, then begins anew
    assert L.dmet_finalize_pending() == 0
    _native.finalize_flush()
    torch.cuda.synchronize()
    for u, v in zip(want, got):
        assert torch.equal(u, v)


@pytest.mark.parametrize("k", [16, 20])
def test_gather_half_form_for_small_event_batches(dev, k):
    """K3: with the batch's largest event known to fit 2 559 rows the LDS gather runs 512-thread workgroups on 80 KB images,
    two to a CU (dmet_gather_max_lds_sliced_cap_f32) -- same (out, arg) bits as the full form; an event BEYOND the hint takes
    the in-kernel L2 path and still comes out right."""
    _default_path_only("DMET_GATHER_MAX_FORM", "l2-only", "the test calls the LDS-resident kernels on slice-major tables directly")
    from deepmetv2_amd import _native
    sizes = [2000, 1, 2559, 700, 33, 1800]
    x, _b, ptr = _ragged(sizes, 32, seed=61)
    xd, pd = x.to(dev), ptr.to(dev)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(32, 64, generator=g) / 8).to(dev)
    b = torch.randn(32, generator=g).to(dev)
    nbr, _d, loc = _native.knn_local(xd, pd, k)
    P, Q = _native.node_linear_split(xd, W, b, sliced=True)
    for want_arg in (True, False):
        full = _native.gather_max(P, Q, nbr, pd, want_arg, lds=True, nbr_local=loc, sliced=True)
        half = _native.gather_max(P, Q, nbr, pd, want_arg, lds=True, nbr_local=loc, sliced=True, max_nodes=max(sizes))
        lied = _native.gather_max(P, Q, nbr, pd, want_arg, lds=True, nbr_local=loc, sliced=True, max_nodes=1000)
        for other in (half, lied):
            assert torch.equal(full[0], other[0])
            assert (full[1] is None) == (other[1] is None) and (full[1] is None or torch.equal(full[1], other[1]))

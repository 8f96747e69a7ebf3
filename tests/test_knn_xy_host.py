"""knn(x, y) / radius(x, y) / the two-set EdgeConv: host-side checks (no GPU needed).

The numpy restatement (tests/knn_xy_reference.py) against what already exists, the argument checks before any device
work, the [2,E] layout over the CPU stand-in, and the two-set EdgeConv / DynamicEdgeConv against plain torch in float64."""
import copy
import math

import numpy as np
import pytest
import torch

import knn_periodic_reference as kp
import knn_xy_reference as xy
import radius_periodic_reference as rp


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _two_sets(seed=0, sx=(30, 0, 5, 1, 12), sy=(7, 9, 0, 1, 40), D=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(sx), D, generator=g)
    y = torch.randn(sum(sy), D, generator=g)
    return x, y, _batch(sx), _batch(sy)


# ---- the reference against what exists -----------------------------------------------------------------------------
@pytest.mark.parametrize("D,k", [(2, 16), (3, 5), (32, 8)])
def test_reference_knn_equals_the_self_query_references(D, k):
    from oracle import ref_ops
    rng = np.random.default_rng(D)
    sizes = [300, 0, 40, 3]
    x = rng.standard_normal((sum(sizes), D)).astype(np.float32)
    if D == 2:
        x = rng.integers(-3, 4, size=x.shape).astype(np.float32)      # lattice: ties at rank k
    ptr = _ptr(sizes)
    nbr, dist = xy.knn_table(x, ptr, x.copy(), ptr, k, None)
    n1, d1, _loc = kp.knn_table(x, ptr, k, None)
    assert np.array_equal(nbr, n1) and np.array_equal(_bits(dist), _bits(d1))
    n2, d2 = ref_ops.knn_table(torch.from_numpy(x), torch.from_numpy(ptr), k)
    assert np.array_equal(nbr, n2.numpy()) and np.array_equal(_bits(dist), _bits(d2.numpy()))


@pytest.mark.parametrize("period", [None, [None, 2 * math.pi]])
def test_reference_radius_equals_the_loop_true_table(period):
    rng = np.random.default_rng(3)
    sizes = [200, 0, 50, 1]
    x = np.stack([rng.uniform(-2, 2, sum(sizes)), rng.uniform(-math.pi, math.pi, sum(sizes))], 1).astype(np.float32)
    ptr = _ptr(sizes)
    for m in (4, 64):
        nbr, cnt = xy.radius_table(x, ptr, x.copy(), ptr, 0.4, m, period)
        n1, c1 = rp.radius_table(x, ptr, 0.4, m, period, skip_self=False)
        assert np.array_equal(nbr, n1) and np.array_equal(cnt, c1)
    assert int((cnt == 64).sum()) == 0 and int((xy.radius_table(x, ptr, x, ptr, 0.4, 4, period)[1] == 4).sum()) > 0


def test_reference_periodic_knn_equals_the_periodic_self_query_reference():
    rng = np.random.default_rng(5)
    x = np.stack([rng.uniform(-2, 2, 150), rng.uniform(-math.pi, math.pi, 150)], 1).astype(np.float32)
    ptr = _ptr([100, 50])
    per = [None, 2 * math.pi]
    nbr, dist = xy.knn_table(x, ptr, x.copy(), ptr, 8, per)
    n1, d1, _ = kp.knn_table(x, ptr, 8, per)
    assert np.array_equal(nbr, n1) and np.array_equal(_bits(dist), _bits(d1))


# ---- argument checks, before any device work -------------------------------------------------------------------------
def _no_native(monkeypatch):
    from deepmetv2_amd import _native

    def boom(*a, **k):
        raise AssertionError("a native entry ran although the arguments are invalid")
    for n in ("knn", "knn_local", "knn_periodic", "knn_xy", "radius_xy", "radius", "radius_periodic"):
        monkeypatch.setattr(_native, n, boom)


def test_argument_checks(monkeypatch):
    import deepmetv2_amd as dm
    xy.install(monkeypatch)
    _no_native(monkeypatch)
    x, y, bx, by = _two_sets()
    for fn, arg in ((dm.knn, 4), (dm.radius, 0.5), (dm.knn_xy_table, 4), (dm.radius_xy_table, 0.5)):
        with pytest.raises(ValueError, match="together"):
            fn(x, y, arg, bx, None)
        with pytest.raises(ValueError, match="together"):
            fn(x, y, arg, None, by)
        with pytest.raises(ValueError, match="sorted"):
            fn(x, y, arg, bx.flip(0).contiguous(), by)
        with pytest.raises(ValueError, match="sorted"):
            fn(x, y, arg, bx, by.flip(0).contiguous())
        with pytest.raises(ValueError, match="coordinates"):
            fn(x, torch.zeros(y.shape[0], 3), arg, bx, by)
        with pytest.raises(ValueError, match="entries"):
            fn(x, y, arg, bx, by, period=[2 * math.pi])
        with pytest.raises(ValueError, match="positive finite"):
            fn(x, y, arg, bx, by, period=[None, -1.0])
        with pytest.raises(TypeError, match="period"):
            fn(x, y, arg, bx, by, period=6.28)
        with pytest.raises(TypeError, match="float32"):
            fn(x.double(), y.double(), arg, bx, by)
    for k in (0, 65, -1, 2.0):
        with pytest.raises(ValueError, match="k"):
            dm.knn(x, y, k, bx, by)
    with pytest.raises(NotImplementedError, match="cosine"):
        dm.knn(x, y, 4, bx, by, cosine=True)
    x9, y9 = torch.zeros(10, 9), torch.zeros(4, 9)
    with pytest.raises(ValueError, match="up to 8 coordinates"):
        dm.knn(x9, y9, 4, period=[None] * 8 + [6.28])
    with pytest.raises(ValueError, match="up to 8 coordinates"):
        dm.radius(x9, y9, 0.5)
    with pytest.raises(ValueError, match="up to 64 coordinates"):
        dm.knn(torch.zeros(10, 65), torch.zeros(4, 65), 4)
    with pytest.raises(ValueError, match="max_num_neighbors"):
        dm.radius(x, y, 0.5, bx, by, max_num_neighbors=0)


# ---- over the stand-in ---------------------------------------------------------------------------------------------
def _expected_edges(x, y, bx, by, k=None, r=None, m=None, period=None, B=None):
    B = B or int(max(bx.max(), by.max())) + 1
    px = _ptr(np.bincount(bx.numpy(), minlength=B))
    py = _ptr(np.bincount(by.numpy(), minlength=B))
    if k is not None:
        return xy.edges_of(xy.knn_table(x.numpy(), px, y.numpy(), py, k, period)[0])
    return xy.edges_of(xy.radius_table(x.numpy(), px, y.numpy(), py, r, m, period)[0])


@pytest.mark.parametrize("period", [None, [None, 2 * math.pi]])
def test_knn_layout_and_order(monkeypatch, period):
    import deepmetv2_amd as dm
    xy.install(monkeypatch)
    x, y, bx, by = _two_sets(1)
    ei = dm.knn(x, y, 8, bx, by, period=period)
    assert ei.dtype == torch.int64 and ei.shape[0] == 2
    assert np.array_equal(ei.numpy(), _expected_edges(x, y, bx, by, k=8, period=period))
    assert int(ei.min()) >= 0                                   # short rows are dropped, never -1
    assert bool((ei[0][1:] >= ei[0][:-1]).all())                # grouped by ascending query
    assert int(ei[0].max()) < y.shape[0] and int(ei[1].max()) < x.shape[0]
    deg = torch.bincount(ei[0], minlength=y.shape[0])
    # events: 30 / 0 / 5 / 1 / 12 candidates against 7 / 9 / 0 / 1 / 40 queries
    assert deg.tolist() == [8] * 7 + [0] * 9 + [1] + [8] * 40
    same_event = bx[ei[1]] == by[ei[0]]
    assert bool(same_event.all())
    table = dm.knn_xy_table(x, y, 8, bx, by, period=period)
    assert table.nbr.shape == (y.shape[0], 8) and table.dist.shape == (y.shape[0], 8)
    assert bool((table.dist[table.nbr < 0] == 1e10).all()) and int((table.nbr < 0).sum()) == 9 * 8 + 7


def test_radius_layout_cap_and_export(monkeypatch):
    import deepmetv2_amd as dm
    assert "radius" in dm.__all__ and callable(dm.radius)
    xy.install(monkeypatch)
    x, y, bx, by = _two_sets(2)
    for m in (3, 32):
        ei = dm.radius(x, y, 0.9, bx, by, max_num_neighbors=m)
        assert np.array_equal(ei.numpy(), _expected_edges(x, y, bx, by, r=0.9, m=m))
        assert int(ei.min()) >= 0 and int(ei[1].max()) < 2 ** 30         # nothing beyond cnt was read
    assert int(torch.bincount(dm.radius(x, y, 0.9, bx, by, max_num_neighbors=3)[0]).max()) == 3      # the cap binds
    t = dm.radius_xy_table(x, y, 0.9, bx, by, max_num_neighbors=3, pad=True)
    assert bool(((t.nbr >= 0) == (torch.arange(3).view(1, -1) < t.cnt.view(-1, 1))).all())


def test_missing_events_and_batch_size(monkeypatch):
    import deepmetv2_amd as dm
    xy.install(monkeypatch)
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(20, 2, generator=g), torch.randn(15, 2, generator=g)
    bx = _batch([10, 0, 10])            # event 1 missing from x, event 3 not there at all
    by = _batch([5, 4, 3, 3])           # y reaches event 3
    ei = dm.knn(x, y, 4, bx, by)
    assert np.array_equal(ei.numpy(), _expected_edges(x, y, bx, by, k=4, B=4))
    assert torch.bincount(ei[0], minlength=15).tolist() == [4] * 5 + [0] * 4 + [4] * 3 + [0] * 3
    by2 = _batch([5, 0, 10])            # event 1 missing from both
    ei2 = dm.knn(x, y, 4, bx, by2, batch_size=6)
    assert np.array_equal(ei2.numpy(), _expected_edges(x, y, bx, by2, k=4, B=6))
    with pytest.raises(ValueError, match="batch values"):
        dm.knn(x, y, 4, bx, by, batch_size=3)
    # no batch vectors: one event
    ei3 = dm.knn(x, y, 4)
    assert np.array_equal(ei3.numpy(), xy.edges_of(xy.knn_table(x.numpy(), [0, 20], y.numpy(), [0, 15], 4)[0]))
    # no queries / no candidates at all
    assert dm.knn(x, y[:0], 4).shape == (2, 0) and dm.knn(x[:0], y, 4).shape == (2, 0)


def test_self_query_keeps_its_route(monkeypatch):
    import fake_native
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    xy.install(monkeypatch)
    calls = []

    def boom(*a, **k):
        raise AssertionError("the two-set entry ran for the self-query form")

    def spy(*a, **k):
        calls.append(a)
        return fake_native.knn_local(*a, **k)
    monkeypatch.setattr(_native, "knn_xy", boom)
    monkeypatch.setattr(_native, "knn_local", spy)
    x, _y, bx, _by = _two_sets(3)
    ei = dm.knn(x, x, 8, bx, bx)
    assert len(calls) == 1 and ei.shape[0] == 2
    assert torch.equal(ei, dm.knn_table(x, 8, bx, loop=True).edge_index("target_to_source"))


# ---- the two-set EdgeConv --------------------------------------------------------------------------------------------
def _nn(kind, F, H):
    torch.manual_seed(7)
    if kind == "linear":
        return torch.nn.Sequential(torch.nn.Linear(2 * F, H))
    return torch.nn.Sequential(torch.nn.Linear(2 * F, 24), torch.nn.ELU(), torch.nn.Linear(24, H), torch.nn.ELU(),
                               torch.nn.BatchNorm1d(H))


def ref_edge_conv_xy(nn64, x_src, x_dst, src, tgt, aggr):
    """Plain torch: out[i] = aggr over the edges (src[e], tgt[e] == i) of nn64([x_dst[i] || x_src[j] - x_dst[i]])."""
    N = x_dst.shape[0]
    msg = nn64(torch.cat([x_dst[tgt], x_src[src] - x_dst[tgt]], 1))
    H = msg.shape[1]
    if aggr == "max":
        out = torch.full((N, H), float("-inf"), dtype=msg.dtype).scatter_reduce(0, tgt.view(-1, 1).expand(-1, H), msg,
                                                                                  "amax", include_self=True)
        return torch.where(torch.isinf(out), torch.zeros_like(out), out)
    out = torch.zeros((N, H), dtype=msg.dtype).index_add(0, tgt, msg)
    if aggr == "mean":
        out = out / torch.bincount(tgt, minlength=N).clamp(min=1).to(out.dtype).view(-1, 1)
    return out


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def check_against_float64(conv, run, x_src, x_dst, src, tgt, aggr, g, rel=1e-4):
    """run(xs, xd) -> out of the module under test; float64 reference over (src, tgt); the bars of the generic-route
    comparisons (tests/test_gpu_short_rows.py): rel x the largest reference magnitude, per layer for the parameters."""
    nn64 = copy.deepcopy(conv.nn).double().cpu()
    xs, xd = x_src.detach().clone().requires_grad_(True), x_dst.detach().clone().requires_grad_(True)
    out = run(xs, xd)
    out.backward(g)
    rs, rd = x_src.detach().cpu().double().requires_grad_(True), x_dst.detach().cpu().double().requires_grad_(True)
    ref = ref_edge_conv_xy(nn64, rs, rd, src.cpu(), tgt.cpu(), aggr)
    ref.backward(g.cpu().double())
    assert out.shape == ref.shape
    for what, a, b in (("out", out, ref), ("g_x_src", xs.grad, rs.grad), ("g_x_dst", xd.grad, rd.grad)):
        a, b = a.detach().cpu().double(), b.detach()
        assert bool(torch.isfinite(a).all()), what
        assert _amax(a - b) <= rel * max(_amax(b), 1e-6), (what, _amax(a - b), _amax(b))
    ref_grads = {n: p.grad for n, p in nn64.named_parameters()}
    scale = {}
    for n, gr in ref_grads.items():
        scale[n.rsplit(".", 1)[0]] = max(scale.get(n.rsplit(".", 1)[0], 0.0), _amax(gr))
    for n, p in conv.nn.named_parameters():
        err = _amax(p.grad.detach().cpu().double() - ref_grads[n])
        assert err <= rel * max(scale[n.rsplit(".", 1)[0]], 1e-6), (n, err)
    return out.detach(), ref.detach()


@pytest.mark.parametrize("aggr", ["max", "add", "sum", "mean"])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
@pytest.mark.parametrize("kind", ["linear", "mlp_bn"])
def test_two_set_edgeconv_against_float64(monkeypatch, aggr, flow, kind):
    import deepmetv2_amd as dm
    xy.install(monkeypatch)
    g = torch.Generator().manual_seed(11)
    F, H, Ns, Nd, E = 6, 5, 23, 17, 90
    x_src, x_dst = torch.randn(Ns, F, generator=g), torch.randn(Nd, F, generator=g)
    src = torch.randint(0, Ns - 2, (E,), generator=g)           # the last two sources: no edge leaves them
    tgt = torch.randint(0, Nd - 3, (E,), generator=g)           # the last three targets: no edge (R3: 0)
    ei = torch.stack([src, tgt] if flow == "source_to_target" else [tgt, src])
    conv = dm.EdgeConv(_nn(kind, F, H), aggr=aggr, flow=flow).train()
    out, ref = check_against_float64(conv, lambda xs, xd: conv((xs, xd), ei), x_src, x_dst, src, tgt, aggr,
                                     torch.randn(Nd, H, generator=g))
    assert out.shape == (Nd, H) and bool((out[-3:] == 0).all())


def test_two_set_edgeconv_checks(monkeypatch):
    import deepmetv2_amd as dm
    xy.install(monkeypatch)
    conv = dm.EdgeConv(_nn("linear", 4, 3))
    xs, xd = torch.randn(5, 4), torch.randn(3, 4)
    with pytest.raises(ValueError, match="features"):
        conv((torch.randn(5, 6), xd), torch.zeros(2, 0, dtype=torch.long))
    with pytest.raises(ValueError, match="source ids"):
        conv((xs, xd), torch.tensor([[5], [0]]))
    with pytest.raises(ValueError, match="target ids"):
        conv((xs, xd), torch.tensor([[4], [3]]))
    with pytest.raises(ValueError, match="source ids"):
        conv((xs, xd), torch.tensor([[-1], [0]]))
    assert conv((xs, xd), torch.tensor([[4], [2]])).shape == (3, 3)           # 4 is a source id: in range for x_src
    assert bool((conv((xs, xd), torch.zeros(2, 0, dtype=torch.long)) == 0).all())
    out_same = conv((xs, xs), torch.tensor([[4], [2]]))                           # a pair of the SAME tensor: one set
    assert torch.equal(out_same, conv(xs, torch.tensor([[4], [2]])))


@pytest.mark.parametrize("aggr", ["max", "mean"])
def test_two_set_dynamic_edgeconv(monkeypatch, aggr):
    import deepmetv2_amd as dm
    xy.install(monkeypatch)
    sx, sy = (12, 0, 3, 9), (4, 5, 6, 0)
    g = torch.Generator().manual_seed(13)
    F, H, k = 3, 4, 5
    x_src, x_dst = torch.randn(sum(sx), F, generator=g), torch.randn(sum(sy), F, generator=g)
    bx, by = _batch(sx), _batch(sy)
    conv = dm.DynamicEdgeConv(_nn("mlp_bn", F, H), k=k, aggr=aggr).train()
    e = xy.edges_of(xy.knn_table(x_src.numpy(), _ptr(sx), x_dst.numpy(), _ptr(sy), k)[0])
    tgt, src = torch.from_numpy(e[0]), torch.from_numpy(e[1])
    out, _ref = check_against_float64(conv, lambda xs, xd: conv((xs, xd), (bx, by)), x_src, x_dst, src, tgt, aggr,
                                      torch.randn(sum(sy), H, generator=g))
    assert bool((out[4:9] == 0).all())                          # the queries of the event without candidates

"""The bf16 matrix-core EdgeConv route for a two-layer edge MLP over any graph (csrc/edgemlp_bf16.hip,
conv._EdgeMLP2Bf16Edges) on the GPU, and the DynamicReductionNetwork under bf16 autocast.

Forward: tight against a torch emulation of the kernel's recipe (P, Q, ELU, aggregation, BatchNorm fp32; h1 and W2
rounded to bf16, exact products, fp32 sums).  Gradients: within the bf16 bar of rule R6 (2e-2 of each layer's gradient
scale) of a float64 composition of the same layer; for max aggregation that composition takes the winners the kernel
picked (a bf16 rounding may reorder two messages within 2^-8 of each other, and the gradient follows the winner)."""
import copy

import pytest
import torch

from edge_mlp_reference import emulate as _emulate, kernel_winners as _kernel_winners, ref64 as _ref64

pytestmark = pytest.mark.gpu

SWITCH = "DMET_EDGE_MLP_BF16"


def _mlp(Hin, H1, H2, act2=True, bias=True, bn=None, neg_gamma=False, seed=0):
    torch.manual_seed(seed)
    mods = [torch.nn.Linear(2 * Hin, H1, bias=bias), torch.nn.ELU(), torch.nn.Linear(H1, H2, bias=bias)]
    if act2:
        mods.append(torch.nn.ELU())
    if bn is not None:
        b = torch.nn.BatchNorm1d(H2)
        with torch.no_grad():
            b.weight.uniform_(0.5, 1.5)
            if neg_gamma:
                b.weight[::2].neg_()
            b.bias.uniform_(-0.5, 0.5)
            b.running_mean.uniform_(-0.2, 0.2)
            b.running_var.uniform_(0.5, 1.5)
        b.train(bn == "train")
        mods.append(b)
    return torch.nn.Sequential(*mods)


def _ragged(sizes, D, seed):
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor(sizes, dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return torch.randn(int(counts.sum()), D, generator=g), batch


def _knn_sym(dev, sizes, k, D, seed=0):
    """ragged events, the DRN's graph: to_undirected(knn_graph(x[:, :32], k, batch, loop=False))"""
    import deepmetv2_amd as dm
    x, batch = _ragged(sizes, D, seed)
    xd, bd = x.to(dev), batch.to(dev)
    ei = dm.to_undirected(dm.knn_graph(xd[:, :32].contiguous(), k, bd, loop=False), num_nodes=xd.shape[0])
    return xd, bd, ei


def _conv(nn, dev, **kw):
    """EdgeConv over a copy of nn with nn's weights and statistics, bf16 compute requested."""
    import deepmetv2_amd as dm
    conv = dm.EdgeConv(copy.deepcopy(nn), **kw)
    conv.nn.load_state_dict(nn.state_dict())
    conv.compute_dtype = torch.bfloat16
    return conv.to(dev)


def _count(monkeypatch, name="edge_mlp_fwd_bf16"):
    """A list that grows by one on every call of _native.<name>."""
    from deepmetv2_amd import _native
    calls = []
    real = getattr(_native, name)
    monkeypatch.setattr(_native, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _run(conv, x, ei, g=None):
    """forward + backward of conv(x, ei): (out, gx, {param: grad}, {buffer: value}, g)"""
    conv.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(True)
    out = conv(xx, ei)
    if g is None:
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    grads = {n: p.grad.detach().clone() for n, p in conv.nn.named_parameters() if p.grad is not None}
    bufs = {n: b.detach().clone() for n, b in conv.nn.named_buffers()}
    return out.detach(), xx.grad.detach().clone(), grads, bufs, g


def _layer_scales(grads):
    """the largest gradient entry per layer (a Linear's bias gradient can be 0 exactly, e.g. before a BatchNorm)"""
    scale = {}
    for n, gr in grads.items():
        layer = n.rsplit(".", 1)[0]
        scale[layer] = max(scale.get(layer, 0.0), _amax(gr))
    return scale


def _check(dev, nn, x, ei, aggr, flow="source_to_target", monkeypatch=None):
    """route taken once; forward tight against the recipe; gradients within R6 of the float64 composition"""
    calls = _count(monkeypatch)
    emu, m = _emulate(nn, x, ei, aggr, flow)
    conv = _conv(nn, dev, aggr=aggr, flow=flow)
    out, gx, grads, bufs, g = _run(conv, x, ei)
    assert len(calls) == 1
    assert out.dtype == torch.float32
    scale = max(_amax(emu), 1e-6)
    assert _amax(out - emu) <= 2e-3 * scale, ("forward vs recipe", _amax(out - emu), scale)
    if aggr == "max":
        grouped, win = _kernel_winners(nn, x, ei, flow)
        r_out, r_gx, r_grads = _ref64(nn, x, grouped, aggr, "source_to_target", g, win)
    else:
        r_out, r_gx, r_grads = _ref64(nn, x, ei, aggr, flow, g)
    assert _amax(out.double() - r_out) <= 2e-2 * max(_amax(r_out), 1e-6), "forward vs float64"
    assert bool(torch.isfinite(gx).all())
    assert _amax(gx.double() - r_gx) <= 2e-2 * max(_amax(r_gx), 1e-6), ("gx", _amax(gx.double() - r_gx), _amax(r_gx))
    assert grads.keys() == r_grads.keys()
    scale = _layer_scales(r_grads)
    for n in r_grads:
        err, sc = _amax(grads[n].double() - r_grads[n]), max(scale[n.rsplit(".", 1)[0]], 1e-6)
        assert bool(torch.isfinite(grads[n]).all()) and err <= 2e-2 * sc, (n, err, sc)
    return out, gx, grads, bufs


# ---- recipe and gradients: widths, aggregations, BatchNorm modes ---------------------------------------------------------
@pytest.mark.parametrize("h", [32, 64, 128])
@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
@pytest.mark.parametrize("bn", [None, "train", "eval"])
def test_drn_widths(dev, monkeypatch, h, aggr, bn):
    x, _b, ei = _knn_sym(dev, [600, 37, 410, 3, 250], 12, h, seed=h)
    _check(dev, _mlp(h, 3 * h // 2, h, bn=bn, seed=h + 1), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_without_second_elu_other_widths(dev, monkeypatch, aggr):
    x, _b, ei = _knn_sym(dev, [500, 300], 10, 48, seed=3)
    _check(dev, _mlp(48, 80, 64, act2=False, bn="train", seed=4), x, ei, aggr, monkeypatch=monkeypatch)
    _check(dev, _mlp(48, 16, 32, act2=False, seed=5), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
@pytest.mark.parametrize("bn", ["train", "eval"])
def test_negative_gamma(dev, monkeypatch, aggr, bn):
    x, _b, ei = _knn_sym(dev, [700, 200], 12, 32, seed=6)
    _check(dev, _mlp(32, 48, 32, bn=bn, neg_gamma=True, seed=7), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "mean"])
def test_biases_none(dev, monkeypatch, aggr):
    x, _b, ei = _knn_sym(dev, [640, 128], 12, 64, seed=8)
    _check(dev, _mlp(64, 96, 64, bias=False, bn="train", seed=9), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_flow_target_to_source(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    x, b = _ragged([500, 400], 32, seed=10)
    x, b = x.to(dev), b.to(dev)
    ei = dm.knn_graph(x, 9, b, loop=False)      # directed: the two flows differ
    _check(dev, _mlp(32, 48, 32, bn="train", seed=11), x, ei, aggr, flow="target_to_source", monkeypatch=monkeypatch)


def test_radius_graph_with_self_loops(dev, monkeypatch):
    import deepmetv2_amd as dm
    x, b = _ragged([800, 300], 64, seed=12)
    x, b = x.to(dev), b.to(dev)
    ei = dm.radius_graph(x[:, :2].contiguous(), 0.4, b, loop=True, max_num_neighbors=255)
    for aggr in ("max", "add"):
        _check(dev, _mlp(64, 96, 64, bn="train", seed=13), x, ei, aggr, monkeypatch=monkeypatch)


# ---- which route is taken --------------------------------------------------------------------------------------------------
def test_route_under_autocast_and_compute_dtype(dev, monkeypatch):
    import deepmetv2_amd as dm
    calls = _count(monkeypatch)
    x, _b, ei = _knn_sym(dev, [300, 200], 8, 32, seed=14)
    conv = _conv(_mlp(32, 48, 32, bn="train", seed=15), dev, aggr="add")
    conv.compute_dtype = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = conv(x, ei)
    assert len(calls) == 1 and out.dtype == torch.float32
    conv.compute_dtype = torch.bfloat16
    conv(x, ei)
    assert len(calls) == 2
    # not taken: fp32 compute, the switch, unsupported widths
    conv.compute_dtype = None
    conv(x, ei)
    conv.compute_dtype = torch.float32
    with torch.autocast("cuda", dtype=torch.bfloat16):
        conv(x, ei)
    assert len(calls) == 2
    conv.compute_dtype = torch.bfloat16
    monkeypatch.setenv(SWITCH, "0")
    conv(x, ei)
    monkeypatch.delenv(SWITCH)
    assert len(calls) == 2
    for nn in (_mlp(32, 48, 16, seed=16), _mlp(32, 40, 32, seed=16)):       # H2 = 16; H1 not a multiple of 16
        c = _conv(nn, dev, aggr="max")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            c(x, ei)
    assert len(calls) == 2
    assert isinstance(dm.EdgeConv(_mlp(32, 48, 32)), torch.nn.Module)


def test_switch_off_gives_the_generic_route(dev, monkeypatch):
    """DMET_EDGE_MLP_BF16=0 under autocast: the generic route (nn under autocast, its bf16 messages upcast for the
    fp32 segment reductions), which supports double backward; the two agree at the R6 bar."""
    x, _b, ei = _knn_sym(dev, [400, 300], 10, 32, seed=17)
    nn = _mlp(32, 48, 32, seed=18)
    conv = _conv(nn, dev, aggr="add")
    conv.compute_dtype = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        fused = conv(x, ei)
        monkeypatch.setenv(SWITCH, "0")
        generic = conv(x, ei)
        monkeypatch.delenv(SWITCH)
    assert fused.dtype == torch.float32 and generic.dtype == torch.float32
    assert _amax(fused - generic) <= 2e-2 * _amax(fused)


def test_existing_table_route_unchanged(dev, monkeypatch):
    """A fixed-width kNN table at a width dmet_edge_mlp2_supported takes still goes to _EdgeMLP2Bf16: same bits as the
    table kernel called directly, and the new route is not called."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    new = _count(monkeypatch)
    old = _count(monkeypatch, "edge_mlp2_bf16")
    x, b = _ragged([700, 300], 32, seed=19)
    x, b = x.to(dev), b.to(dev)
    nn = _mlp(32, 48, 32, seed=20)
    assert _native.edge_mlp2_supported(32, 48, 32, 16)
    conv = dm.DynamicEdgeConv(copy.deepcopy(nn), k=16, aggr="max").to(dev)
    conv.nn.load_state_dict(nn.state_dict())
    conv.compute_dtype = torch.bfloat16
    out = conv(x, b)
    assert len(old) == 1 and len(new) == 0
    table = dm.knn_table(x, 16, b, loop=True)
    l1, l2 = conv.nn[0], conv.nn[2]
    direct = _native.edge_mlp2_bf16(x, table.nbr, l1.weight, l1.bias, l2.weight, l2.bias, True, False)
    assert torch.equal(out, direct)


# ---- determinism, BatchNorm statistics -------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits(dev):
    x, _b, ei = _knn_sym(dev, [900, 700, 300], 12, 64, seed=21)
    for aggr in ("max", "add", "mean"):
        conv = _conv(_mlp(64, 96, 64, bn="train", neg_gamma=True, seed=22), dev, aggr=aggr)
        a = _run(conv, x, ei)
        b = _run(conv, x, ei, a[4])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), aggr
        for n in a[2]:
            assert torch.equal(a[2][n], b[2][n]), (aggr, n)


def test_running_stats_move_once_per_step(dev):
    x, _b, ei = _knn_sym(dev, [500, 300], 10, 32, seed=23)
    nn = _mlp(32, 48, 32, bn="train", seed=24)
    conv = _conv(nn, dev, aggr="add")
    _emu, m = _emulate(torch.nn.Sequential(*list(conv.nn)[:-1]), x, ei, "add", "source_to_target")   # messages before the norm
    bn = conv.nn[-1]
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    E = m.shape[0]
    _run(conv, x, ei)
    assert int(bn.num_batches_tracked) == 1
    # the messages' batch statistics, moved once with momentum 0.1 (unbiased variance)
    mean, var = m.double().mean(0), m.double().var(0, unbiased=True)
    exp_m = (0.9 * rm0.double() + 0.1 * mean).float()
    exp_v = (0.9 * rv0.double() + 0.1 * var).float()
    torch.testing.assert_close(bn.running_mean, exp_m, rtol=2e-3, atol=2e-3 * _amax(exp_m))
    torch.testing.assert_close(bn.running_var, exp_v, rtol=2e-3, atol=2e-3 * _amax(exp_v))
    _run(conv, x, ei)
    assert int(bn.num_batches_tracked) == 2 and E > 1


# ---- edge cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [None, "eval"])
def test_no_edges(dev, monkeypatch, bn):
    x = torch.randn(50, 32, device=dev)
    ei = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    conv = _conv(_mlp(32, 48, 32, bn=bn, seed=25), dev, aggr="max")
    out, gx, grads, _bufs, _g = _run(conv, x, ei)
    assert torch.equal(out, torch.zeros_like(out)) and torch.equal(gx, torch.zeros_like(gx))
    for n, gr in grads.items():
        assert torch.equal(gr, torch.zeros_like(gr)), n


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
def test_nodes_without_in_edges(dev, monkeypatch, aggr):
    """half of the nodes receive no edge: their output is 0, their gradient only what their out-edges give"""
    g = torch.Generator().manual_seed(26)
    N = 600
    src = torch.randint(0, N, (4000,), generator=g)
    tgt = torch.randint(0, N // 2, (4000,), generator=g) * 2        # even targets only
    ei = torch.stack([src, tgt]).to(dev)
    x = torch.randn(N, 32, generator=g).to(dev)
    out, *_ = _check(dev, _mlp(32, 48, 32, bn="train", seed=27), x, ei, aggr, monkeypatch=monkeypatch)
    assert torch.equal(out[1::2], torch.zeros_like(out[1::2]))


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_hub_above_one_tile(dev, monkeypatch, aggr):
    """a hub whose in-degree (1500) spans many 32-edge tiles and several workgroups, next to ordinary nodes"""
    g = torch.Generator().manual_seed(28)
    N = 2000
    hub_src = torch.arange(1, 1501)
    src = torch.cat([hub_src, torch.randint(0, N, (6000,), generator=g)])
    tgt = torch.cat([torch.zeros(1500, dtype=torch.int64), torch.randint(0, N, (6000,), generator=g)])
    ei = torch.stack([src, tgt]).to(dev)
    x = torch.randn(N, 64, generator=g).to(dev)
    _check(dev, _mlp(64, 96, 64, bn="train", seed=29), x, ei, aggr, monkeypatch=monkeypatch)


# ---- memory --------------------------------------------------------------------------------------------------------------------
def test_memory_stays_below_a_quarter_of_the_edge_features(dev, monkeypatch):
    """8 x 4000 nodes, k 32, hidden 64, forward + backward under autocast: peak growth below a quarter of one
    [E, 2 Hin] fp32 tensor (the bound of the fp32 route's test).  The generic route (DMET_EDGE_MLP_BF16=0) is far
    above it."""
    x, _b, ei = _knn_sym(dev, [4000] * 8, 32, 64, seed=30)
    E = ei.shape[1]
    bound = E * 64 * 2
    grown = {}
    for route in ("bf16", "generic"):
        if route == "generic":
            monkeypatch.setenv(SWITCH, "0")
        conv = _conv(_mlp(64, 96, 64, bn="train", seed=31), dev, aggr="add")
        conv.compute_dtype = None
        xx = x.detach().clone().requires_grad_(True)
        g = torch.randn(x.shape[0], 64, device=dev)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.max_memory_allocated(dev)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = conv(xx, ei)
        out.float().backward(g)
        torch.cuda.synchronize(dev)
        grown[route] = torch.cuda.max_memory_allocated(dev) - base
        assert bool(torch.isfinite(xx.grad).all())
        del out, xx
    monkeypatch.delenv(SWITCH)
    assert grown["bf16"] < bound, (grown, bound)
    assert grown["generic"] > 2 * bound, (grown, bound)


# ---- bf16 features ---------------------------------------------------------------------------------------------------------------
def test_knn_graph_of_bf16_features(dev):
    import deepmetv2_amd as dm
    x, b = _ragged([900, 17, 400], 32, seed=32)
    xb, bd = x.to(dev).to(torch.bfloat16), b.to(dev)
    for loop in (False, True):
        assert torch.equal(dm.knn_graph(xb, 16, bd, loop=loop), dm.knn_graph(xb.float(), 16, bd, loop=loop))
    with pytest.raises(TypeError):
        dm.knn_graph(x.to(dev).half(), 16, bd)


def test_edge_conv_takes_bf16_features(dev, monkeypatch):
    """a bf16 x is upcast on entry: the output is the layer's on x.float(), the gradient reaches x in bf16"""
    calls = _count(monkeypatch)
    x, _b, ei = _knn_sym(dev, [500, 300], 10, 32, seed=33)
    xb = x.to(torch.bfloat16)
    conv = _conv(_mlp(32, 48, 32, seed=34), dev, aggr="max")
    xr = xb.detach().clone().requires_grad_(True)
    out = conv(xr, ei)
    out.sum().backward()
    assert len(calls) == 1 and xr.grad is not None and xr.grad.dtype == torch.bfloat16
    assert torch.equal(out, conv(xb.float(), ei))


# ---- the whole DRN under autocast ------------------------------------------------------------------------------------------------
def _drn_data(dev, n_events, n_nodes, seed):
    x, batch = _ragged([n_nodes] * n_events, 5, seed=seed)
    data = type("D", (), {})()
    data.x, data.batch = x.to(dev), batch.to(dev)
    return data


def _drn_step(m, data, seeds, autocast, conv_dtype=None):
    for conv in (m.edgeconv1, m.edgeconv2):
        conv.compute_dtype = conv_dtype
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = m(data, seeds=seeds)
    out.float().sum().backward()
    return out.detach().float(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_drn_under_autocast_against_fp32(dev, monkeypatch):
    """4 x 1000, hidden 64: forward and backward under bf16 autocast take the new route in both EdgeConvs.  Every run
    after the first replays the fp32 run's kNN graphs and graclus clusters, so that the runs differ in precision only.

    Measured on MI355X (max |diff| / max |fp32 output|): the DRN with only its EdgeConvs on the bf16 route 0.9 %, within
    the R6 bar; under full autocast 2.6 %, of which torch's own bf16 recipe for the input and output Linears is the
    larger part -- the generic route under autocast (DMET_EDGE_MLP_BF16=0, torch's recipe for the edge MLP too) is at
    3.5 %.  Whole-model parameter gradients are not held to R6: through the max pools and the BatchNorm over the
    messages any bf16 recipe moves them by several percent (inputnet.0.bias: 37 % under autocast with this route, 66 %
    with torch's recipe); the edge-MLP layer's own gradients are held to R6 by the tests above."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import drn
    rec = {"knn_graph": [], "graclus": []}
    pos = {"knn_graph": 0, "graclus": 0}
    replay = [False]

    def recorded(name, fn):
        def call(*a, **k):
            if replay[0]:
                pos[name] += 1
                return rec[name][pos[name] - 1]
            r = fn(*a, **k)
            rec[name].append(r)
            return r
        return call
    monkeypatch.setattr(drn, "knn_graph", recorded("knn_graph", drn.knn_graph))
    monkeypatch.setattr(drn, "graclus", recorded("graclus", drn.graclus))
    calls = _count(monkeypatch)
    torch.manual_seed(35)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev)
    data = _drn_data(dev, 4, 1000, seed=36)
    ref, ref_g = _drn_step(m, data, (11, 12), autocast=False)
    assert len(calls) == 0 and len(rec["knn_graph"]) == 2 and len(rec["graclus"]) == 2
    replay[0] = True

    def run(**kw):
        pos.update(knn_graph=0, graclus=0)
        out, grads = _drn_step(m, data, (11, 12), **kw)
        assert pos == {"knn_graph": 2, "graclus": 2}
        assert bool(torch.isfinite(out).all()) and grads.keys() == ref_g.keys()
        for n, gr in grads.items():
            assert bool(torch.isfinite(gr).all()), n
        return _amax(out - ref) / max(_amax(ref), 1e-6)
    err_route = run(autocast=False, conv_dtype=torch.bfloat16)
    assert len(calls) == 2
    assert err_route <= 2e-2, err_route
    err_autocast = run(autocast=True)
    assert len(calls) == 4
    monkeypatch.setenv(SWITCH, "0")
    err_torch = run(autocast=True)
    monkeypatch.delenv(SWITCH)
    assert len(calls) == 4
    assert err_autocast <= err_torch, (err_autocast, err_torch)


def test_drn_under_autocast_full_size(dev, monkeypatch):
    """64 x 4500, hidden 64, k 16 (the DRN's shape): forward + backward under bf16 autocast, no graph pinned; both
    EdgeConvs take the new route, output and every parameter gradient finite."""
    import deepmetv2_amd as dm
    calls = _count(monkeypatch)
    torch.manual_seed(37)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev)
    data = _drn_data(dev, 64, 4500, seed=38)
    out, grads = _drn_step(m, data, (13, 14), autocast=True)
    assert len(calls) == 2
    assert out.shape == (64,) and bool(torch.isfinite(out).all())
    assert grads
    for n, gr in grads.items():
        assert bool(torch.isfinite(gr).all()), n

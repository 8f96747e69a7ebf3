"""The fused fp32 EdgeConv route for a two-layer edge MLP (csrc/edgemlp_f32.hip, conv._EdgeMLP2F32) on the GPU, against
the CPU oracle (oracle.ref_ops.edge_conv) and against the generic route (DMET_EDGE_MLP_F32=0)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = "DMET_EDGE_MLP_F32"


def _mlp(Hin, H1, H2, act2=True, bias=True, bn=None, neg_gamma=False, track=True, seed=0):
    torch.manual_seed(seed)
    mods = [torch.nn.Linear(2 * Hin, H1, bias=bias), torch.nn.ELU(), torch.nn.Linear(H1, H2, bias=bias)]
    if act2:
        mods.append(torch.nn.ELU())
    if bn is not None:
        b = torch.nn.BatchNorm1d(H2, track_running_stats=track)
        with torch.no_grad():
            b.weight.uniform_(0.5, 1.5)
            if neg_gamma:
                b.weight[::2].neg_()
            b.bias.uniform_(-0.5, 0.5)
            if track:
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
    import deepmetv2_amd as dm
    x, batch = _ragged(sizes, D, seed)
    xd, bd = x.to(dev), batch.to(dev)
    ei = dm.to_undirected(dm.knn_graph(xd[:, :32].contiguous(), k, bd, loop=False), num_nodes=xd.shape[0])
    return xd, bd, ei


def _conv(nn, dev, **kw):
    """EdgeConv over a copy of nn with nn's weights and statistics (EdgeConv.__init__ resets its nn, as PyG's does)."""
    import deepmetv2_amd as dm
    conv = dm.EdgeConv(copy.deepcopy(nn), **kw)
    conv.nn.load_state_dict(nn.state_dict())
    return conv.to(dev)


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _run(conv, x, ei, g=None):
    """forward + backward of conv(x, ei): (out, gx, {param name: grad}, {buffer name: value})."""
    conv.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(True)
    out = conv(xx, ei)
    if g is None:
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    grads = {n: p.grad.detach().clone() for n, p in conv.nn.named_parameters() if p.grad is not None}
    bufs = {n: b.detach().clone() for n, b in conv.nn.named_buffers()}
    return out.detach(), xx.grad.detach().clone(), grads, bufs, g


def _run_cpu(nn_cpu, x, ei, aggr, flow, g):
    from oracle import ref_ops
    xx = x.detach().cpu().clone().requires_grad_(True)
    out = ref_ops.edge_conv(xx, ei.cpu(), nn_cpu, aggr, flow=flow)
    out.backward(g.cpu())
    grads = {n: p.grad.detach().clone() for n, p in nn_cpu.named_parameters() if p.grad is not None}
    bufs = {n: b.detach().clone() for n, b in nn_cpu.named_buffers()}
    return out.detach(), xx.grad.detach().clone(), grads, bufs


def _layer_scales(grads):
    scale = {}
    for n, gr in grads.items():
        layer = n.rsplit(".", 1)[0]
        scale[layer] = max(scale.get(layer, 0.0), float(gr.abs().max()))
    return scale


def _close(a, b, what):
    """a, b: (out, gx, grads) -- output within 1e-4 of its scale, every gradient within 1e-4 of its layer's scale."""
    out_a, gx_a, gr_a = a[0].cpu(), a[1].cpu(), {n: v.cpu() for n, v in a[2].items()}
    out_b, gx_b, gr_b = b[0].cpu(), b[1].cpu(), {n: v.cpu() for n, v in b[2].items()}
    assert bool(torch.isfinite(out_a).all()) and bool(torch.isfinite(gx_a).all()), what
    assert _amax(out_a - out_b) <= 1e-4 * max(_amax(out_b), 1e-6), (what, "out")
    assert _amax(gx_a - gx_b) <= 1e-4 * max(_amax(gx_b), 1e-6), (what, "gx")
    assert gr_a.keys() == gr_b.keys(), what
    scale = _layer_scales(gr_b)
    for n in gr_b:
        tol = 1e-4 * max(scale[n.rsplit(".", 1)[0]], 1e-6)
        err = float((gr_a[n] - gr_b[n]).abs().max())
        assert bool(torch.isfinite(gr_a[n]).all()) and err <= tol, (what, n, err, tol)


def _count_fused(monkeypatch):
    """A list that grows by one on every call of the fused route's forward entry."""
    from deepmetv2_amd import _native
    calls = []
    real = _native.edge_mlp_fwd_f32
    monkeypatch.setattr(_native, "edge_mlp_fwd_f32", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _check_route(dev, nn, x, ei, aggr, flow="source_to_target", monkeypatch=None, expect_fused=True):
    """fused route vs the CPU oracle and vs the generic route; the BatchNorm buffers of all three move alike."""
    calls = _count_fused(monkeypatch)
    nn_cpu = copy.deepcopy(nn)
    conv = _conv(nn, dev, aggr=aggr, flow=flow)
    fused = _run(conv, x, ei)
    assert len(calls) == (1 if expect_fused else 0)
    monkeypatch.setenv(SWITCH, "0")
    conv_g = _conv(nn, dev, aggr=aggr, flow=flow)
    generic = _run(conv_g, x, ei, fused[4])
    monkeypatch.delenv(SWITCH)
    assert len(calls) == (1 if expect_fused else 0)
    ref = _run_cpu(nn_cpu, x, ei, aggr, flow, fused[4])
    _close(fused, ref, "vs oracle")
    _close(fused, generic, "vs generic")
    for n, b in ref[3].items():
        fb, gb = fused[3][n].cpu(), generic[3][n].cpu()
        if b.dtype == torch.int64:
            assert torch.equal(fb, b) and torch.equal(gb, b), n
        else:
            torch.testing.assert_close(fb, b, rtol=1e-5, atol=1e-6, msg=n)
    return fused, generic


# ---- coverage: aggregations, act2, BatchNorm modes, widths ----------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["max", "add", "sum", "mean"])
@pytest.mark.parametrize("act2", [True, False])
@pytest.mark.parametrize("bn", [None, "train", "eval"])
def test_coverage_hidden16(dev, monkeypatch, aggr, act2, bn):
    x, _b, ei = _knn_sym(dev, [60, 3, 0, 41], 6, 16, seed=1)
    nn = _mlp(16, 24, 16, act2=act2, bn=bn, seed=2)
    _check_route(dev, nn, x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
@pytest.mark.parametrize("bn", [None, "train"])
def test_coverage_hidden64(dev, monkeypatch, aggr, bn):
    x, _b, ei = _knn_sym(dev, [90, 40], 8, 64, seed=3)
    nn = _mlp(64, 96, 64, bn=bn, seed=4)
    _check_route(dev, nn, x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("h", [32, 128])
def test_coverage_other_drn_widths(dev, monkeypatch, h):
    x, _b, ei = _knn_sym(dev, [70, 25], 6, h, seed=5)
    nn = _mlp(h, 3 * h // 2, h, bn="train", seed=6)
    _check_route(dev, nn, x, ei, "add", monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_biases_none(dev, monkeypatch, aggr):
    x, _b, ei = _knn_sym(dev, [50, 30], 5, 16, seed=7)
    _check_route(dev, _mlp(16, 24, 16, bias=False, seed=8), x, ei, aggr, monkeypatch=monkeypatch)
    _check_route(dev, _mlp(16, 24, 16, bias=False, bn="train", seed=8), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("bn", ["train", "eval"])
@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
def test_negative_gamma(dev, monkeypatch, bn, aggr):
    """a < 0 on every other channel: max takes the minimum's branch, and its winner."""
    x, _b, ei = _knn_sym(dev, [70, 20], 6, 16, seed=9)
    _check_route(dev, _mlp(16, 24, 16, bn=bn, neg_gamma=True, seed=10), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_batchnorm_without_running_stats(dev, monkeypatch, aggr):
    x, _b, ei = _knn_sym(dev, [64, 33], 6, 16, seed=11)
    _check_route(dev, _mlp(16, 24, 16, bn="train", track=False, seed=12), x, ei, aggr, monkeypatch=monkeypatch)


def test_running_stats_move_once_per_step(dev):
    import deepmetv2_amd as dm
    x, _b, ei = _knn_sym(dev, [80, 50], 6, 16, seed=13)
    nn = _mlp(16, 24, 16, bn="train", seed=14)
    conv = _conv(nn, dev, aggr="add")
    ref = copy.deepcopy(nn)
    from oracle import ref_ops
    for step in range(3):
        _run(conv, x, ei)
        ref_ops.edge_conv(x.cpu(), ei.cpu(), ref, "add").sum().backward()
        bn_g, bn_c = conv.nn[-1], ref[-1]
        assert int(bn_g.num_batches_tracked) == step + 1 == int(bn_c.num_batches_tracked)
        torch.testing.assert_close(bn_g.running_mean.cpu(), bn_c.running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(bn_g.running_var.cpu(), bn_c.running_var, rtol=1e-5, atol=1e-6)


def test_unsupported_width_keeps_the_generic_bits(dev, monkeypatch):
    from deepmetv2_amd import _native
    calls = []
    real = _native.edge_mlp_fwd_f32
    monkeypatch.setattr(_native, "edge_mlp_fwd_f32", lambda *a, **k: calls.append(1) or real(*a, **k))
    x, _b, ei = _knn_sym(dev, [40, 20], 5, 16, seed=15)
    nn = _mlp(16, 36, 24, bn="train", seed=16)         # H2 = 24: outside dmet_edge_mlp_f32_supported
    assert not _native.edge_mlp_f32_supported(16, 36, 24)
    a = _run(_conv(nn, dev, aggr="add"), x, ei)
    monkeypatch.setenv(SWITCH, "0")
    b = _run(_conv(nn, dev, aggr="add"), x, ei, a[4])
    assert calls == []
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def test_radius_graph_with_self_loops(dev, monkeypatch):
    import deepmetv2_amd as dm
    x, batch = _ragged([120, 60], 16, seed=17)
    xd, bd = x.to(dev), batch.to(dev)
    ei = dm.radius_graph(xd[:, :2] * 0.5, 0.4, bd, loop=True, max_num_neighbors=255)
    for aggr in ("max", "add"):
        _check_route(dev, _mlp(16, 24, 16, bn="train", seed=18), xd, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "mean"])
def test_flow_target_to_source(dev, monkeypatch, aggr):
    x, _b, ei = _knn_sym(dev, [50, 30], 5, 16, seed=19)
    ei = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(0)).to(dev)][:, : ei.shape[1] * 2 // 3]
    _check_route(dev, _mlp(16, 24, 16, bn="train", seed=20), x, ei, aggr, flow="target_to_source",
                 monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
def test_nodes_without_in_edges(dev, monkeypatch, aggr):
    g = torch.Generator().manual_seed(21)
    N = 70
    src = torch.randint(0, N, (300,), generator=g)
    tgt = torch.randint(0, N // 2, (300,), generator=g) * 2          # odd nodes and some even ones receive nothing
    ei = torch.stack([src, tgt]).to(dev)
    x = torch.randn(N, 16, generator=g).to(dev)
    fused, _gen = _check_route(dev, _mlp(16, 24, 16, bn="train", seed=22), x, ei, aggr, monkeypatch=monkeypatch)
    assert bool((fused[0][1::2] == 0).all())


@pytest.mark.parametrize("bn", [None, "eval"])
def test_no_edges(dev, monkeypatch, bn):
    """E = 0: every output is 0 (R3) and every gradient is 0 (the generic route's output has no autograd graph here)."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    calls = []
    real = _native.edge_mlp_fwd_f32
    monkeypatch.setattr(_native, "edge_mlp_fwd_f32", lambda *a, **k: calls.append(1) or real(*a, **k))
    x = torch.randn(12, 16).to(dev)
    ei = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    conv = _conv(_mlp(16, 24, 16, bn=bn, seed=23), dev, aggr="add")
    out, gx, grads, _bufs, _g = _run(conv, x, ei)
    assert calls == [1]
    assert out.shape == (12, 16) and bool((out == 0).all()) and bool((gx == 0).all())
    for n, gr in grads.items():
        assert bool((gr == 0).all()), n
    monkeypatch.setenv(SWITCH, "0")
    assert torch.equal(_conv(_mlp(16, 24, 16, bn=bn, seed=23), dev, aggr="add")(x, ei), out)


@pytest.mark.parametrize("bn", [None, "eval"])
def test_empty_input(dev, monkeypatch, bn):
    """N = 0: out is [0, H2] like the generic route's, and every gradient is 0."""
    calls = _count_fused(monkeypatch)
    x = torch.zeros((0, 16), device=dev)
    ei = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    nn = _mlp(16, 24, 16, bn=bn, seed=37)
    out, gx, grads, bufs, _g = _run(_conv(nn, dev, aggr="max"), x, ei)
    assert calls == [1]
    assert out.shape == (0, 16) and gx.shape == (0, 16)
    assert sorted(grads) == sorted(n for n, _p in nn.named_parameters())
    for n, gr in grads.items():
        assert bool((gr == 0).all()), n
    for n, b in nn.named_buffers():
        assert torch.equal(bufs[n].cpu(), b), n
    monkeypatch.setenv(SWITCH, "0")
    assert _conv(nn, dev, aggr="max")(x, ei).shape == (0, 16)


def test_batchnorm_training_over_one_edge_keeps_the_generic_route(dev, monkeypatch):
    import deepmetv2_amd as dm
    x = torch.randn(3, 16).to(dev)
    ei = torch.tensor([[0], [1]], device=dev)
    conv = _conv(_mlp(16, 24, 16, bn="train", seed=24), dev, aggr="add")
    with pytest.raises(ValueError):
        conv(x, ei)


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_star_hub_above_255(dev, monkeypatch, aggr):
    N = 700
    g = torch.Generator().manual_seed(25)
    spokes = torch.arange(1, N)
    src = torch.cat([spokes, torch.zeros(N - 1, dtype=torch.int64), torch.randint(1, N, (400,), generator=g)])
    tgt = torch.cat([torch.zeros(N - 1, dtype=torch.int64), spokes, torch.randint(1, N, (400,), generator=g)])
    ei = torch.stack([src, tgt]).to(dev)
    x = torch.randn(N, 16, generator=g).to(dev)
    _check_route(dev, _mlp(16, 24, 16, bn="train", seed=26), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("bn", [None, "train"])
def test_duplicate_nodes_max_ties(dev, monkeypatch, bn):
    """Exact duplicates give exactly tied messages: the gradient must reach the node the generic route picks."""
    x, _b, ei = _knn_sym(dev, [40], 6, 16, seed=27)
    x = torch.cat([x, x[:10]])                  # nodes 40..49 duplicate 0..9
    N = x.shape[0]
    extra = torch.stack([torch.arange(40, 50), torch.arange(10, 20)]).to(dev)   # 40+i and i both feed 10+i
    extra2 = torch.stack([torch.arange(0, 10), torch.arange(10, 20)]).to(dev)
    ei = torch.cat([extra, ei, extra2], dim=1)
    fused, generic = _check_route(dev, _mlp(16, 24, 16, bn=bn, seed=28), x, ei, "max", monkeypatch=monkeypatch)
    assert N == 50
    assert torch.equal(fused[1][40:] != 0, generic[1][40:] != 0)


def test_dynamic_edge_conv_table_path(dev, monkeypatch):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    x, batch = _ragged([80, 5, 50], 16, seed=29)
    xd, bd = x.to(dev), batch.to(dev)
    nn = _mlp(16, 24, 16, bn="train", seed=30)
    conv = dm.DynamicEdgeConv(copy.deepcopy(nn), k=8, aggr="add")
    conv.nn.load_state_dict(nn.state_dict())
    conv = conv.to(dev)
    calls = _count_fused(monkeypatch)
    xx = xd.clone().requires_grad_(True)
    out = conv(xx, bd)
    assert calls == [1]          # the table path's fall-through takes the fused route
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(6))
    out.backward(g.to(dev))
    ref_nn = copy.deepcopy(nn)
    xc = x.clone().requires_grad_(True)
    ref = ref_ops.dynamic_edge_conv(xc, batch, ref_nn, 8, "add")
    ref.backward(g)
    grads = {n[3:]: p.grad for n, p in conv.named_parameters()}
    ref_grads = {n: p.grad for n, p in ref_nn.named_parameters()}
    _close((out.detach(), xx.grad, grads), (ref.detach(), xc.grad, ref_grads), "DynamicEdgeConv")


# ---- determinism, memory, the DRN -----------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits(dev):
    import deepmetv2_amd as dm
    x, _b, ei = _knn_sym(dev, [900, 700, 300], 12, 64, seed=31)
    for aggr in ("max", "add"):
        conv = _conv(_mlp(64, 96, 64, bn="train", neg_gamma=True, seed=32), dev, aggr=aggr)
        a = _run(conv, x, ei)
        b = _run(conv, x, ei, a[4])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for n in a[2]:
            assert torch.equal(a[2][n], b[2][n]), n


def test_memory_stays_below_a_quarter_of_the_edge_features(dev):
    """The bound is a quarter of one [E, 2 Hin] fp32 tensor.  Measured by tools/edge_mlp_memory.py on this graph
    (profiles/edge_mlp_f32_memory.json): the fused route grows by 0.65x the bound, the generic route by 18.5x (its
    per-edge tensors: edge features, both Linears, ELUs, BatchNorm)."""
    import deepmetv2_amd as dm
    x, _b, ei = _knn_sym(dev, [4000] * 8, 32, 64, seed=33)
    E = ei.shape[1]
    conv = _conv(_mlp(64, 96, 64, bn="train", seed=34), dev, aggr="add")
    xx = x.detach().clone().requires_grad_(True)
    g = torch.randn(x.shape[0], 64, device=dev)
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.max_memory_allocated(dev)
    out = conv(xx, ei)
    out.backward(g)
    torch.cuda.synchronize(dev)
    grown = torch.cuda.max_memory_allocated(dev) - base
    assert grown < E * 64 * 2, (grown, E * 64 * 2)
    assert bool(torch.isfinite(xx.grad).all())


def test_drn_full_size_against_the_generic_route(dev, monkeypatch):
    """64 x 4500, hidden 64, k 16, forward + backward on the fused route against the same model on the generic route.

    The second run replays the first run's kNN graphs and graclus matchings, so that the two runs differ only in the
    EdgeConv route (a near-tie in a kNN distance or a matching weight would otherwise let rounding change the graph).
    The gradients of the two edge MLPs are checked against a float64 composition of the same layer on the same inputs
    instead: there the generic fp32 route is itself up to 7e-4 of the layer scale away from float64 (its BatchNorm and
    weight-gradient sums over ~3 M edge rows), the fused route about 1e-5."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import drn
    from oracle import ref_ops
    rec = {"knn_graph": [], "graclus": []}
    replay = [False]

    def recorded(name, fn):
        def call(*a, **k):
            if replay[0]:
                return rec[name].pop(0)
            r = fn(*a, **k)
            rec[name].append(r)
            return r
        return call
    monkeypatch.setattr(drn, "knn_graph", recorded("knn_graph", drn.knn_graph))
    monkeypatch.setattr(drn, "graclus", recorded("graclus", drn.graclus))
    torch.manual_seed(35)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16)
    m_gen = copy.deepcopy(m).to(dev)
    m = m.to(dev)
    cap = {}
    for name in ("edgeconv1", "edgeconv2"):
        def pre(mod, args, name=name):
            cap[name] = (args[0].detach().clone(), args[1])

        def post(mod, args, out, name=name):
            out.register_hook(lambda gr, name=name: cap.__setitem__(name + "_g", gr.detach().clone()))
        getattr(m, name).register_forward_pre_hook(pre)
        getattr(m, name).register_forward_hook(post)
    x, batch = _ragged([4500] * 64, 5, seed=36)
    ptr = torch.arange(0, 64 * 4500 + 1, 4500)
    data = type("D", (), {})()
    data.x, data.batch = x.to(dev), batch.to(dev)
    dm.register_batch(data.batch, ptr.to(dev), 64, max_nodes=4500, min_nodes=4500)
    calls = _count_fused(monkeypatch)
    out = m(data, seeds=(1, 2))
    out.sum().backward()
    assert calls == [1, 1]       # both EdgeConvs on the fused route
    replay[0] = True
    monkeypatch.setenv(SWITCH, "0")
    out_g = m_gen(data, seeds=(1, 2))
    out_g.sum().backward()
    monkeypatch.delenv(SWITCH)
    assert calls == [1, 1]
    assert not rec["knn_graph"] and not rec["graclus"]
    assert bool(torch.isfinite(out).all())
    assert _amax(out - out_g) <= 1e-4 * max(_amax(out_g), 1e-6)
    grads = {n: p.grad for n, p in m.named_parameters()}
    ref = {n: p.grad for n, p in m_gen.named_parameters()}
    # the edge MLPs: float64 composition of the layer on the inputs and output gradient the fused run saw
    for name in ("edgeconv1", "edgeconv2"):
        xi, ei = cap[name]
        n64 = copy.deepcopy(getattr(m_gen, name).nn).double().cpu()
        n64.train()
        ref_ops.edge_conv(xi.double().cpu(), ei.cpu(), n64, "add").backward(cap[name + "_g"].double().cpu())
        for n, p in n64.named_parameters():
            ref[f"{name}.nn.{n}"] = p.grad.float().to(dev)
    scale = _layer_scales(ref)
    for n in ref:
        assert bool(torch.isfinite(grads[n]).all()), n
        tol = 1e-4 * max(scale[n.rsplit(".", 1)[0]], 1e-6)
        err = _amax(grads[n] - ref[n])
        assert err <= tol, (n, err, tol)

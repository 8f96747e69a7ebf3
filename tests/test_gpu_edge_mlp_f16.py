"""The fp16 matrix-core EdgeConv route for a two-layer edge MLP over any graph (csrc/edgemlp_bf16.hip instantiated for
fp16, conv._EdgeMLP2F16Edges) on the GPU, and the operators that take fp16 inputs.

Linear configuration (act2=False, aggr='add', no BatchNorm): every output and weight gradient within 1e-5 of the sum of
the magnitudes of its terms of a float64 sum over the fp16-rounded operands (torch's .half(): round to nearest even,
subnormals kept).  The recipe with ELU, BatchNorm and every aggregation: forward tight against a torch emulation (P, Q,
ELU, aggregation, BatchNorm fp32; h1 and W2 rounded to fp16, exact products, fp32 sums), gradients within 5e-3 of each
layer's gradient scale of a float64 composition (a quarter of the R6 bar the bf16 route is held to)."""
import copy

import pytest
import torch

from edge_mlp_reference import ends as _ends, ref64 as _ref64

pytestmark = pytest.mark.gpu

SWITCH = "DMET_EDGE_MLP_F16"
GRAD_BAR = 5e-3


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
    """EdgeConv over a copy of nn with nn's weights and statistics, fp16 compute requested."""
    import deepmetv2_amd as dm
    conv = dm.EdgeConv(copy.deepcopy(nn), **kw)
    conv.nn.load_state_dict(nn.state_dict())
    conv.compute_dtype = torch.float16
    return conv.to(dev)


def _count(monkeypatch, name="edge_mlp_fwd_f16"):
    """A list that grows by one on every call of _native.<name>."""
    from deepmetv2_amd import _native
    calls = []
    real = getattr(_native, name)
    monkeypatch.setattr(_native, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _h(t):
    """fp16 rounding as torch does it (RNE, subnormals kept), as float64"""
    return t.half().double()


def _emulate(nn, x, ei, aggr, flow):
    """The kernel's recipe in torch: (out, post-BatchNorm messages [E, H2]).  P and Q are formed in float64 and kept as
    fp32, h1 = ELU(P_tgt + Q_src) in fp32, z2 from fp16(h1) and fp16(W2) (exact products, float64 sums, kept as fp32)."""
    mods = list(copy.deepcopy(nn).to(x.device))
    bn = mods.pop() if isinstance(mods[-1], torch.nn.BatchNorm1d) else None
    l1, l2, act2 = mods[0], mods[2], len(mods) == 4
    tgt, src = _ends(ei, flow)
    N, Hin = x.shape
    with torch.no_grad():
        W1 = l1.weight.double()
        b1 = l1.bias.double() if l1.bias is not None else 0.0
        xd = x.double()
        P = (xd @ (W1[:, :Hin] - W1[:, Hin:]).T + b1).float()
        Q = (xd @ W1[:, Hin:].T).float()
        h1 = torch.nn.functional.elu(P[tgt] + Q[src])
        z = (_h(h1) @ _h(l2.weight).T).float()
        if l2.bias is not None:
            z = z + l2.bias
        m = torch.nn.functional.elu(z) if act2 else z
        if bn is not None:
            if bn.training:
                mean, var = m.double().mean(0), m.double().var(0, unbiased=False)
            else:
                mean, var = bn.running_mean.double(), bn.running_var.double()
            a = bn.weight.double() / torch.sqrt(var + bn.eps)
            m = (a * m.double() + (bn.bias.double() - mean * a)).float()
        H2 = m.shape[1]
        idx = tgt.view(-1, 1).expand(-1, H2)
        if aggr == "max":
            out = torch.zeros((N, H2), dtype=m.dtype, device=m.device).scatter_reduce(0, idx, m, "amax", include_self=False)
        else:
            out = torch.zeros((N, H2), dtype=m.dtype, device=m.device).index_add_(0, tgt, m)
            if aggr == "mean":
                out = out / torch.bincount(tgt, minlength=N).clamp(min=1).to(m.dtype).view(-1, 1)
    return out, m


def _kernel_winners(nn, x, ei, flow):
    """(grouped edge index [2, E], winners [N, H2]) as the fp16 kernel's forward state records them (-1: no in-edge)"""
    from deepmetv2_amd import _native
    from deepmetv2_amd.conv import _as_mlp2
    from deepmetv2_amd.graph import edge_list_from_edge_index
    l1, l2, act2, bn = _as_mlp2(copy.deepcopy(nn).to(x.device))
    edges = edge_list_from_edge_index(ei, x.shape[0], flow)
    mode = 0 if bn is None else (1 if bn.training else 2)
    _out, (_pq, _agg, win, bnstat) = _native.edge_mlp_fwd_f16(
        x, edges.rowptr, edges.src, edges.tgt, l1.weight, l1.bias, l2.weight, l2.bias, act2, "max", mode,
        bn.weight if bn is not None else None, bn.bias if bn is not None else None, 1e-5, 0.1,
        bn.running_mean if mode == 2 else None, bn.running_var if mode == 2 else None, None)
    w = win[0].long()
    if mode:
        w = torch.where(bnstat[0] < 0, win[1].long(), w)
    deg = (edges.rowptr[1:] - edges.rowptr[:-1]).view(-1, 1)
    grouped = torch.stack([edges.src.long(), edges.tgt.long()])
    return grouped, torch.where(deg > 0, w, torch.full_like(w, -1))


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
    scale = {}
    for n, gr in grads.items():
        layer = n.rsplit(".", 1)[0]
        scale[layer] = max(scale.get(layer, 0.0), _amax(gr))
    return scale


def _check(dev, nn, x, ei, aggr, flow="source_to_target", monkeypatch=None):
    """route taken once; forward tight against the recipe; gradients within GRAD_BAR of the float64 composition"""
    calls = _count(monkeypatch)
    bwd = _count(monkeypatch, "edge_mlp_bwd_f16")
    emu, _m = _emulate(nn, x, ei, aggr, flow)
    conv = _conv(nn, dev, aggr=aggr, flow=flow)
    out, gx, grads, bufs, g = _run(conv, x, ei)
    assert len(calls) == 1 and len(bwd) == 1
    assert out.dtype == torch.float32
    scale = max(_amax(emu), 1e-6)
    assert _amax(out - emu) <= 1e-3 * scale, ("forward vs recipe", _amax(out - emu), scale)
    if aggr == "max":
        grouped, win = _kernel_winners(nn, x, ei, flow)
        r_out, r_gx, r_grads = _ref64(nn, x, grouped, aggr, "source_to_target", g, win)
    else:
        r_out, r_gx, r_grads = _ref64(nn, x, ei, aggr, flow, g)
    assert _amax(out.double() - r_out) <= GRAD_BAR * max(_amax(r_out), 1e-6), "forward vs float64"
    assert bool(torch.isfinite(gx).all())
    assert _amax(gx.double() - r_gx) <= GRAD_BAR * max(_amax(r_gx), 1e-6), ("gx", _amax(gx.double() - r_gx), _amax(r_gx))
    assert grads.keys() == r_grads.keys()
    scale = _layer_scales(r_grads)
    for n in r_grads:
        err, sc = _amax(grads[n].double() - r_grads[n]), max(scale[n.rsplit(".", 1)[0]], 1e-6)
        assert bool(torch.isfinite(grads[n]).all()) and err <= GRAD_BAR * sc, (n, err, sc)
    return out, gx, grads, bufs


# ---- the linear configuration against float64 sums over the fp16-rounded operands -----------------------------------------------
def _rtz(t):
    """fp32 -> fp16 rounded toward zero (what v_cvt_pkrtz_f16_f32 does), as float64: one step toward zero where RNE
    rounded away (sign-magnitude bits: minus one is one step toward zero for either sign; +-inf becomes +-65504)"""
    h = t.half()
    away = h.double().abs() > t.double().abs()
    bits = h.view(torch.int16)
    return torch.where(away, bits - 1, bits).view(torch.float16).double()


def _linear_case(dev, g_scale=1.0):
    from deepmetv2_amd import _native
    from deepmetv2_amd.graph import edge_list_from_edge_index
    x, _b, ei = _knn_sym(dev, [600, 37, 410, 3, 250], 12, 64, seed=40)
    nn = _mlp(64, 96, 64, act2=False, seed=41).to(dev)
    l1, l2 = nn[0], nn[2]
    edges = edge_list_from_edge_index(ei, x.shape[0], "source_to_target")
    out, state = _native.edge_mlp_fwd_f16(x, edges.rowptr, edges.src, edges.tgt, l1.weight, l1.bias, l2.weight, l2.bias,
                                          False, "add", 0)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(42)).to(dev) * g_scale
    srcptr, srcperm = edges.by_source()
    grads = _native.edge_mlp_bwd_f16(g, x, edges.rowptr, edges.src, edges.tgt, srcptr, srcperm, l1.weight, l2.weight,
                                     l2.bias, False, "add", 0, state)
    pq = state[0]
    H1 = l1.out_features
    tgt, src = edges.tgt.long(), edges.src.long()
    with torch.no_grad():
        h1 = torch.nn.functional.elu(pq[tgt, :H1] + pq[src, H1:])      # fp32, from the kernel's own P and Q
    return x, edges, l2, h1, g[tgt], out, grads


def test_linear_forward_within_the_fp32_sum_of_rounded_operands(dev):
    x, edges, l2, h1, _gz, out, _grads = _linear_case(dev)
    N, H2 = out.shape
    tgt = edges.tgt.long()
    b2 = l2.bias.detach().double()
    for rnd, name in ((_h, "rne"), (_rtz, "rtz")):
        a, w = rnd(h1), rnd(l2.weight.detach())
        terms = a @ w.T + b2
        mags = a.abs() @ w.abs().T + b2.abs()
        ref = torch.zeros((N, H2), dtype=torch.float64, device=dev).index_add_(0, tgt, terms)
        bound = 1e-5 * torch.zeros((N, H2), dtype=torch.float64, device=dev).index_add_(0, tgt, mags)
        excess = float(((out.double() - ref).abs() - bound).max())
        if name == "rne":
            assert excess <= 0.0, excess
        else:
            # the same sum over round-toward-zero operands misses the bound: the test tells the two conversions apart
            assert excess > 0.0, excess


@pytest.mark.parametrize("g_scale", [1.0, 2.0 ** -18])
def test_linear_weight_gradient_within_the_fp32_sum_of_rounded_operands(dev, g_scale):
    """gW2 = sum_e fp16(g_z2[e])^T fp16(h1[e]).  At g_scale 2^-18 most g_z2 values are fp16 subnormals (below 6.1e-5):
    the float64 reference keeps them, so a flush to zero on the way into the matrix cores would miss the bound."""
    _x, _edges, l2, h1, gz, _out, grads = _linear_case(dev, g_scale)
    gW2, gb2 = grads[3], grads[4]
    a, b = _h(gz), _h(h1)
    if g_scale < 1.0:
        sub = (a != 0) & (a.abs() < 2.0 ** -14)
        assert float(sub.double().mean()) > 0.5
    ref = a.T @ b
    bound = 1e-5 * (a.abs().T @ b.abs())
    assert bool(((gW2.double() - ref).abs() <= bound).all()), float(((gW2.double() - ref).abs() - bound).max())
    assert _amax(gb2.double() - gz.double().sum(0)) <= 1e-5 * float(gz.double().abs().sum(0).max())


def test_overflow_goes_to_inf_not_to_the_largest_finite(dev):
    """g_z2 beyond 65504 after rounding: gW2 comes out non-finite, never a saturated finite value"""
    _x, _edges, _l2, _h1, gz, _out, grads = _linear_case(dev, 2.0 ** 20)
    assert float(gz.abs().max()) > 65520.0
    assert not bool(torch.isfinite(grads[3]).all())


# ---- recipe and gradients: widths, aggregations, BatchNorm modes ---------------------------------------------------------
@pytest.mark.parametrize("h", [32, 64, 128])
@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
@pytest.mark.parametrize("bn", [None, "train", "eval"])
def test_drn_widths(dev, monkeypatch, h, aggr, bn):
    x, _b, ei = _knn_sym(dev, [600, 37, 410, 3, 250], 12, h, seed=h)
    _check(dev, _mlp(h, 3 * h // 2, h, bn=bn, seed=h + 1), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
@pytest.mark.parametrize("bn", ["train", "eval"])
def test_negative_gamma(dev, monkeypatch, aggr, bn):
    x, _b, ei = _knn_sym(dev, [700, 200], 12, 32, seed=6)
    _check(dev, _mlp(32, 48, 32, bn=bn, neg_gamma=True, seed=7), x, ei, aggr, monkeypatch=monkeypatch)


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_flow_target_to_source_without_bias(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    x, b = _ragged([500, 400], 32, seed=10)
    x, b = x.to(dev), b.to(dev)
    ei = dm.knn_graph(x, 9, b, loop=False)      # directed: the two flows differ
    _check(dev, _mlp(32, 48, 32, bias=False, bn="train", seed=11), x, ei, aggr, flow="target_to_source",
           monkeypatch=monkeypatch)


# ---- which route is taken --------------------------------------------------------------------------------------------------
def test_route_under_autocast_and_compute_dtype(dev, monkeypatch):
    calls = _count(monkeypatch)
    bf16 = _count(monkeypatch, "edge_mlp_fwd_bf16")
    x, _b, ei = _knn_sym(dev, [300, 200], 8, 32, seed=14)
    conv = _conv(_mlp(32, 48, 32, bn="train", seed=15), dev, aggr="add")
    conv.compute_dtype = None
    with torch.autocast("cuda"):                    # no dtype: float16
        out = conv(x, ei)
    assert len(calls) == 1 and out.dtype == torch.float32
    conv.compute_dtype = torch.float16
    conv(x, ei)
    assert len(calls) == 2
    with torch.autocast("cuda", dtype=torch.bfloat16):  # compute_dtype wins over autocast
        conv(x, ei)
    assert len(calls) == 3 and len(bf16) == 0
    conv.compute_dtype = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        conv(x, ei)
    assert len(calls) == 3 and len(bf16) == 1
    # not taken: fp32 compute, the switch
    conv(x, ei)
    conv.compute_dtype = torch.float32
    with torch.autocast("cuda"):
        conv(x, ei)
    conv.compute_dtype = torch.float16
    monkeypatch.setenv(SWITCH, "0")
    conv(x, ei)
    monkeypatch.delenv(SWITCH)
    assert len(calls) == 3


def test_table_route_stays_bf16_only(dev, monkeypatch):
    """DynamicEdgeConv over a fixed-width kNN table under fp16: the table kernel (bf16 only) is not called, the layer
    reads the table's edge list on the new route"""
    import deepmetv2_amd as dm
    new = _count(monkeypatch)
    old = _count(monkeypatch, "edge_mlp2_bf16")
    x, b = _ragged([700, 300], 32, seed=19)
    x, b = x.to(dev), b.to(dev)
    nn = _mlp(32, 48, 32, seed=20)
    conv = dm.DynamicEdgeConv(copy.deepcopy(nn), k=16, aggr="max").to(dev)
    conv.nn.load_state_dict(nn.state_dict())
    with torch.autocast("cuda"):
        out = conv(x, b)
    assert len(old) == 0 and len(new) == 1 and out.dtype == torch.float32
    table = dm.knn_table(x, 16, b, loop=True)
    ei = table.edge_index("source_to_target")
    emu, _m = _emulate(nn, x, ei, "max", "source_to_target")
    assert _amax(out - emu) <= 1e-3 * _amax(emu)


def test_switch_off_gives_the_generic_route(dev, monkeypatch):
    """DMET_EDGE_MLP_F16=0 under fp16 autocast: the generic route (nn under autocast, its fp16 messages upcast for the
    fp32 segment reductions); the two agree at the R6 bar"""
    x, _b, ei = _knn_sym(dev, [400, 300], 10, 32, seed=17)
    conv = _conv(_mlp(32, 48, 32, seed=18), dev, aggr="add")
    conv.compute_dtype = None
    generic_calls = _count(monkeypatch, "segment_sum")
    with torch.autocast("cuda"):
        fused = conv(x, ei)
        assert len(generic_calls) == 0
        monkeypatch.setenv(SWITCH, "0")
        generic = conv(x, ei)
        monkeypatch.delenv(SWITCH)
    assert len(generic_calls) == 1
    assert fused.dtype == torch.float32 and generic.dtype == torch.float32
    assert _amax(fused - generic) <= 2e-2 * _amax(fused)


# ---- determinism, edge cases, memory ---------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits(dev):
    x, _b, ei = _knn_sym(dev, [900, 700, 300], 12, 64, seed=21)
    for aggr in ("max", "add", "mean"):
        conv = _conv(_mlp(64, 96, 64, bn="train", neg_gamma=True, seed=22), dev, aggr=aggr)
        a = _run(conv, x, ei)
        b = _run(conv, x, ei, a[4])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), aggr
        for n in a[2]:
            assert torch.equal(a[2][n], b[2][n]), (aggr, n)


@pytest.mark.parametrize("bn", [None, "eval"])
def test_no_edges(dev, bn):
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
    src = torch.cat([torch.arange(1, 1501), torch.randint(0, N, (6000,), generator=g)])
    tgt = torch.cat([torch.zeros(1500, dtype=torch.int64), torch.randint(0, N, (6000,), generator=g)])
    ei = torch.stack([src, tgt]).to(dev)
    x = torch.randn(N, 64, generator=g).to(dev)
    _check(dev, _mlp(64, 96, 64, bn="train", seed=29), x, ei, aggr, monkeypatch=monkeypatch)


def test_memory_stays_below_a_quarter_of_the_edge_features(dev, monkeypatch):
    """8 x 4000 nodes, k 32, hidden 64, forward + backward under fp16 autocast: peak growth below a quarter of one
    [E, 2 Hin] fp32 tensor.  The generic route (DMET_EDGE_MLP_F16=0) is far above it."""
    x, _b, ei = _knn_sym(dev, [4000] * 8, 32, 64, seed=30)
    E = ei.shape[1]
    bound = E * 64 * 2
    grown = {}
    for route in ("f16", "generic"):
        if route == "generic":
            monkeypatch.setenv(SWITCH, "0")
        conv = _conv(_mlp(64, 96, 64, bn="train", seed=31), dev, aggr="add")
        conv.compute_dtype = None
        xx = x.detach().clone().requires_grad_(True)
        g = torch.randn(x.shape[0], 64, device=dev)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.max_memory_allocated(dev)
        with torch.autocast("cuda"):
            out = conv(xx, ei)
        out.float().backward(g)
        torch.cuda.synchronize(dev)
        grown[route] = torch.cuda.max_memory_allocated(dev) - base
        assert bool(torch.isfinite(xx.grad).all())
        del out, xx
    monkeypatch.delenv(SWITCH)
    assert grown["f16"] < bound, (grown, bound)
    assert grown["generic"] > 2 * bound, (grown, bound)


# ---- operators that take fp16 ------------------------------------------------------------------------------------------------------
def test_knn_graph_of_16bit_features(dev):
    """under fp16 autocast the graph builders take fp16 features: the indices are those of x.float(); outside fp16
    autocast an fp16 x still raises"""
    import deepmetv2_amd as dm
    x, b = _ragged([900, 17, 400], 32, seed=32)
    x, bd = x.to(dev), b.to(dev)
    xh = x.half()
    xf = xh.float()
    with torch.autocast("cuda"):
        for loop in (False, True):
            assert torch.equal(dm.knn_graph(xh, 16, bd, loop=loop), dm.knn_graph(xf, 16, bd, loop=loop))
        assert torch.equal(dm.knn(xh, xh, 16, bd, bd), dm.knn(xf, xf, 16, bd, bd))
        assert torch.equal(dm.knn_table(xh, 16, bd).nbr, dm.knn_table(xf, 16, bd).nbr)
        pos = x[:, :2].contiguous().half()
        assert torch.equal(dm.radius_graph(pos, 0.4, bd, loop=True, max_num_neighbors=64),
                           dm.radius_graph(pos.float(), 0.4, bd, loop=True, max_num_neighbors=64))
    for ctx in (torch.autocast("cuda", enabled=False), torch.autocast("cuda", dtype=torch.bfloat16)):
        with ctx, pytest.raises(TypeError):
            dm.knn_graph(xh, 16, bd)


def test_edge_conv_takes_fp16_features(dev, monkeypatch):
    """with fp16 requested (compute_dtype or fp16 autocast) an fp16 x is upcast on entry: the output is the layer's on
    x.float(), the gradient reaches x in fp16"""
    import deepmetv2_amd as dm
    calls = _count(monkeypatch)
    x, b, ei = _knn_sym(dev, [500, 300], 10, 32, seed=33)
    xh = x.half()
    conv = _conv(_mlp(32, 48, 32, seed=34), dev, aggr="max")
    xr = xh.detach().clone().requires_grad_(True)
    out = conv(xr, ei)
    out.sum().backward()
    assert len(calls) == 1 and xr.grad is not None and xr.grad.dtype == torch.float16
    assert torch.equal(out, conv(xh.float(), ei))
    dyn = dm.DynamicEdgeConv(copy.deepcopy(conv.nn), k=8, aggr="add").to(dev)
    xr = xh.detach().clone().requires_grad_(True)
    with pytest.raises(TypeError):
        dyn(xr, b)                  # no fp16 requested: an fp16 x stays an error
    with torch.autocast("cuda"):
        out = dyn(xr, b)
        again = dyn(xh.float(), b)
    out.sum().backward()
    assert xr.grad.dtype == torch.float16 and torch.equal(out, again)


def test_scatter_ops_take_16bit_src(dev):
    """scatter_add / scatter_max of bf16 and fp16 src: fp32 sums / maxima by the deterministic kernels, returned in
    src.dtype as torch_scatter returns them; gradients come back in src.dtype"""
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(44)
    batch = torch.sort(torch.randint(0, 5, (3000,), generator=g)).values.to(dev)
    idx2 = torch.randint(0, 400, (6000,), generator=g).to(dev)
    for dt in (torch.bfloat16, torch.float16):
        s1 = torch.randn(3000, generator=g).to(dev).to(dt).requires_grad_(True)
        r = dm.scatter_add(s1, batch)
        assert r.dtype == dt and torch.equal(r, dm.scatter_add(s1.detach().float(), batch).to(dt))
        r.float().sum().backward()
        assert s1.grad.dtype == dt
        s2 = torch.randn(6000, 16, generator=g).to(dev).to(dt).requires_grad_(True)
        r = dm.scatter_add(s2, idx2, dim=0, dim_size=400)
        assert r.dtype == dt and torch.equal(r, dm.scatter_add(s2.detach().float(), idx2, dim=0, dim_size=400).to(dt))
        mx, arg = dm.scatter_max(s2, idx2, dim=0, dim_size=400)
        mx32, arg32 = dm.scatter_max(s2.detach().float(), idx2, dim=0, dim_size=400)
        assert mx.dtype == dt and torch.equal(mx.float(), mx32) and torch.equal(arg, arg32)
        mx.float().sum().backward()
        assert s2.grad.dtype == dt


def test_met_reduce_and_loss_take_16bit_weights(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from deepmetv2_amd.model import loss_fn
    x, y, batch, _ptr = synth.make_events([500, 90, 700], seed=45, device=dev)
    w = torch.rand(x.shape[0], generator=torch.Generator().manual_seed(46)).to(dev)
    for dt in (torch.bfloat16, torch.float16):
        wh = w.to(dt).requires_grad_(True)
        met = dm.met_reduce(wh, x, batch)
        assert met.dtype == torch.float32 and torch.equal(met, dm.met_reduce(wh.detach().float(), x, batch))
        loss = loss_fn(wh, x, y, batch)
        assert loss.dtype == torch.float32
        assert torch.equal(loss, loss_fn(wh.detach().float(), x, y, batch))
        loss.backward()
        assert wh.grad.dtype == dt and bool(torch.isfinite(wh.grad).all())

"""The fused EdgeConv route for a single Linear message with aggr 'add' / 'sum' / 'mean' (csrc/edgeconv_sum.hip,
conv._EdgeConvLinearSum) on the GPU: float64 parity over every graph form, exact properties, routing, no host sync, memory."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = "DMET_EDGE_LINEAR_SUM"
WIDTHS = [(32, 32), (64, 64), (32, 64), (64, 32)]


def _lin(Hin, Hout, bias=True, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(2 * Hin, Hout, bias=bias))


def _conv(nn, dev, cls=None, **kw):
    """EdgeConv / DynamicEdgeConv over a copy of nn with nn's weights (the constructor resets its nn, as PyG's does)."""
    import deepmetv2_amd as dm
    conv = (cls or dm.EdgeConv)(copy.deepcopy(nn), **kw)
    conv.nn.load_state_dict(nn.state_dict())
    return conv.to(dev)


def _ragged(sizes, D, seed):
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor(sizes, dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return torch.randn(int(counts.sum()), D, generator=g), batch


def _count(monkeypatch):
    """Calls of the route's forward entries (table and CSR form) and of the generic route's edge features."""
    from deepmetv2_amd import _native
    calls = {"table": 0, "csr": 0, "edge_features": 0}
    for name, key in (("gather_sum_table", "table"), ("gather_sum_csr", "csr"), ("edge_features", "edge_features")):
        real = getattr(_native, name)

        def wrapped(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(_native, name, wrapped)
    return calls


def _run(conv, x, graph, g=None, *args):
    """forward + backward: (out, gx, {param name: grad}, g)."""
    conv.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(True)
    out = conv(xx, graph, *args)
    if g is None:
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    grads = {n: p.grad.detach().clone() for n, p in conv.nn.named_parameters()}
    return out.detach(), xx.grad.detach().clone(), grads, g


def _edge_conv64(x, ei, nn, aggr, flow):
    """ref_ops.edge_conv restated for device tensors (its scatter_add is CPU-only): the full-size case runs in float64 on
    the GPU, where the [E, 2F] float64 features of 4.6 M edges take seconds instead of minutes."""
    i_row, j_row = (1, 0) if flow == "source_to_target" else (0, 1)
    tgt, src = ei[i_row], ei[j_row]
    msg = nn(torch.cat([x[tgt], x[src] - x[tgt]], -1))
    out = torch.zeros((x.shape[0], msg.shape[1]), dtype=msg.dtype, device=x.device).index_add(0, tgt, msg)
    if aggr == "mean":
        out = out / torch.bincount(tgt, minlength=x.shape[0]).clamp(min=1).to(out.dtype).view(-1, 1)
    return out


def _ref(nn, x, ei, aggr, flow, g, on_device=False):
    """float64 oracle (oracle.ref_ops.edge_conv on the CPU; on_device: _edge_conv64) on double copies, plus the per-row
    bar sum_e |message|_inf."""
    from oracle import ref_ops
    d = x.device if on_device else torch.device("cpu")
    nn64 = copy.deepcopy(nn).double().to(d)
    xx = x.detach().to(d).double().clone().requires_grad_(True)
    ei = ei.to(d)
    fn = _edge_conv64 if on_device else ref_ops.edge_conv
    out = fn(xx, ei, nn64, aggr, flow=flow)
    out.backward(g.to(d).double())
    with torch.no_grad():
        i_row, j_row = (1, 0) if flow == "source_to_target" else (0, 1)
        tgt, src = ei[i_row], ei[j_row]
        msg = nn64(torch.cat([xx[tgt], xx[src] - xx[tgt]], -1)).abs().amax(1) if ei.shape[1] else xx.new_zeros(0)
        bar = torch.zeros(x.shape[0], dtype=torch.float64, device=d).index_add_(0, tgt, msg)
    grads = {n: p.grad.detach() for n, p in nn64.named_parameters()}
    return out.detach(), xx.grad.detach(), grads, bar


def _check(got, ref, what):
    r_out, r_gx, r_grads, bar = ref
    d = r_out.device
    out, gx, grads = got[0].to(d).double(), got[1].to(d).double(), {n: v.to(d) for n, v in got[2].items()}
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all()), what
    err = (out - r_out).abs().amax(1) if out.numel() else torch.zeros(0, dtype=torch.float64, device=out.device)
    lim = 1e-5 * bar + 1e-6
    assert bool((err <= lim).all()), (what, "out", float((err - lim).max()))
    for name, a, b in [("gx", gx, r_gx)] + [(n, grads[n].double(), r_grads[n]) for n in r_grads]:
        scale = max(float(b.abs().max()) if b.numel() else 0.0, 1e-6)
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * scale, msg=f"{what}: {name}")


def _parity(dev, nn, x, graph, ei, aggr, flow="source_to_target", monkeypatch=None, form=None, cls=None,
            on_device=False, **kw):
    """Route taken (form 'table' or 'csr'), no edge features, and float64 parity of out, gx, gW, gb."""
    calls = _count(monkeypatch)
    conv = _conv(nn, dev, cls=cls, aggr=aggr, flow=flow, **kw)
    got = _run(conv, x, graph)
    if form is not None:
        assert calls[form] == 1 and calls["table" if form == "csr" else "csr"] == 0, calls
    assert calls["edge_features"] == 0, calls
    _check(got, _ref(nn, x, ei, aggr, flow, got[3], on_device), f"{aggr} {form}")
    return got


def _knn_inputs(dev, sizes, D, seed):
    x, batch = _ragged(sizes, D, seed)
    return x.to(dev), batch.to(dev)


# ---- 1. parity against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["add", "sum", "mean"])
@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("bias", [True, False])
def test_knn_graph_widths(dev, monkeypatch, aggr, widths, bias):
    import deepmetv2_amd as dm
    Hin, Hout = widths
    x, batch = _knn_inputs(dev, [300, 7, 200], Hin, seed=1)
    ei = dm.knn_graph(x, 12, batch, loop=True)
    _parity(dev, _lin(Hin, Hout, bias, seed=2), x, ei, ei, aggr, monkeypatch=monkeypatch, form="table")


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_knn_graph_flows_and_loops(dev, monkeypatch, aggr, loop, flow):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [250, 120, 9], 32, seed=3)
    ei = dm.knn_graph(x, 16, batch, loop=loop, flow=flow)
    _parity(dev, _lin(32, 32, seed=4), x, ei, ei, aggr, flow=flow, monkeypatch=monkeypatch, form="table")


@pytest.mark.parametrize("aggr", ["add", "sum", "mean"])
@pytest.mark.parametrize("widths", [(32, 32), (64, 32)])
def test_dynamic_edge_conv_ragged(dev, monkeypatch, aggr, widths):
    import deepmetv2_amd as dm
    Hin, Hout = widths
    x, batch = _knn_inputs(dev, [80, 5, 50, 1, 130], Hin, seed=5)
    ei = dm.knn_graph(x, 8, batch, loop=True)           # the graph DynamicEdgeConv builds (same kernel)
    _parity(dev, _lin(Hin, Hout, seed=6), x, batch, ei, aggr, monkeypatch=monkeypatch, form="table",
            cls=dm.DynamicEdgeConv, k=8)


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_knn_table_passed_directly(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [400, 33], 64, seed=7)
    table = dm.knn_table(x, 20, batch, loop=False)
    ei = table.edge_list()
    ei = torch.stack([ei.src.long(), ei.tgt.long()])
    _parity(dev, _lin(64, 64, seed=8), x, table, ei, aggr, monkeypatch=monkeypatch, form="table")


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("as_table", [True, False])
def test_radius_graph_and_table(dev, monkeypatch, aggr, loop, as_table):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(9)
    sizes = [600, 300]
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes)).to(dev)
    pos = (torch.rand(sum(sizes), 2, generator=g) * 3).to(dev)
    x = torch.randn(sum(sizes), 32, generator=g).to(dev)
    if as_table:
        table = dm.radius_table(pos, 0.4, batch, loop=loop, max_num_neighbors=255)
        el = table.edge_list()
        graph, ei = table, torch.stack([el.src.long(), el.tgt.long()])
    else:
        graph = ei = dm.radius_graph(pos, 0.4, batch, loop=loop, max_num_neighbors=255)
    assert ei.shape[1] > 0
    _parity(dev, _lin(32, 64, seed=10), x, graph, ei, aggr, monkeypatch=monkeypatch, form="table")


@pytest.mark.parametrize("aggr", ["add", "sum", "mean"])
@pytest.mark.parametrize("widths", [(32, 32), (64, 32)])
def test_unsorted_edge_index_with_duplicates(dev, monkeypatch, aggr, widths):
    Hin, Hout = widths
    g = torch.Generator().manual_seed(11)
    N = 300
    ei = torch.randint(0, N, (2, 2500), generator=g)
    ei = torch.cat([ei, ei[:, :400]], 1)                 # duplicate edges
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].to(dev)
    x = torch.randn(N, Hin, generator=g).to(dev)
    _parity(dev, _lin(Hin, Hout, seed=12), x, ei, ei, aggr, monkeypatch=monkeypatch, form="csr")


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_star_hub_above_255(dev, monkeypatch, aggr):
    N = 700
    g = torch.Generator().manual_seed(13)
    spokes = torch.arange(1, N)
    src = torch.cat([spokes, torch.zeros(N - 1, dtype=torch.int64), torch.randint(1, N, (400,), generator=g)])
    tgt = torch.cat([torch.zeros(N - 1, dtype=torch.int64), spokes, torch.randint(1, N, (400,), generator=g)])
    ei = torch.stack([src, tgt]).to(dev)
    x = torch.randn(N, 64, generator=g).to(dev)
    _parity(dev, _lin(64, 64, seed=14), x, ei, ei, aggr, monkeypatch=monkeypatch, form="csr")


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_nodes_without_in_edges(dev, monkeypatch, aggr):
    g = torch.Generator().manual_seed(15)
    N = 200
    ei = torch.randint(0, N, (2, 900), generator=g)
    ei = ei[:, ei[1] % 3 != 0].to(dev)                   # every third node receives nothing
    x = torch.randn(N, 32, generator=g).to(dev)
    got = _parity(dev, _lin(32, 32, seed=16), x, ei, ei, aggr, monkeypatch=monkeypatch, form="csr")
    assert bool((got[0][::3] == 0).all())


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_no_edges(dev, monkeypatch, aggr):
    calls = _count(monkeypatch)
    x = torch.randn(12, 32).to(dev)
    ei = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    out, gx, grads, _g = _run(_conv(_lin(32, 32, seed=17), dev, aggr=aggr), x, ei)
    assert calls["csr"] == 1 and calls["edge_features"] == 0
    assert out.shape == (12, 32) and bool((out == 0).all()) and bool((gx == 0).all())
    for n, gr in grads.items():
        assert bool((gr == 0).all()), n


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_empty_input(dev, monkeypatch, aggr):
    calls = _count(monkeypatch)
    x = torch.zeros((0, 32), device=dev)
    ei = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    out, gx, grads, _g = _run(_conv(_lin(32, 64, seed=18), dev, aggr=aggr), x, ei)
    assert calls["csr"] == 1
    assert out.shape == (0, 64) and gx.shape == (0, 32)
    for n, gr in grads.items():
        assert bool((gr == 0).all()), n


# ---- 2. exact properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_empty_rows_are_exactly_zero_where_p_is_not_finite(dev, monkeypatch, aggr):
    g = torch.Generator().manual_seed(19)
    N = 64
    ei = torch.randint(2, N, (2, 400), generator=g).to(dev)  # nodes 0 and 1: no edge in or out
    x = torch.randn(N, 32, generator=g)
    x[0, 3] = float("inf")
    x[1, 5] = float("nan")
    x = x.to(dev)
    calls = _count(monkeypatch)
    out, gx, grads, _g = _run(_conv(_lin(32, 32, seed=20), dev, aggr=aggr), x, ei)
    assert calls["csr"] == 1
    assert bool((out[:2] == 0).all()) and not bool(torch.signbit(out[:2]).any())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all())
    for n, gr in grads.items():
        assert bool(torch.isfinite(gr).all()), n


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_full_rows_knn_table_with_a_nan_query(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()
    x, batch = _ragged([120, 90], 32, seed=21)
    x[7, 2] = float("nan")
    xd, bd = x.to(dev), batch.to(dev)
    table = dm.knn_table(xd, 8, bd, loop=True)
    assert table.full_rows
    calls = _count(monkeypatch)
    conv = _conv(_lin(32, 32, seed=22), dev, aggr=aggr)
    out, gx, grads, g = _run(conv, xd, table)
    assert calls["table"] == 1 and calls["edge_features"] == 0
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all())
    for n, gr in grads.items():
        assert bool(torch.isfinite(gr).all()), n
    from deepmetv2_amd import _native
    P, Q = _native.node_linear_split(xd, conv.nn[0].weight.detach(), conv.nn[0].bias.detach())
    _o, deg = _native.gather_sum_table(P, Q, table.nbr, table.cnt, aggr == "mean")
    assert torch.equal(deg.long(), (table.nbr >= 0).sum(1))
    assert int(deg[7]) == 0 and bool((out[7] == 0).all())
    # the other rows against float64 over the valid edges; the NaN row reads nothing and nobody reads it
    el = table.edge_list()
    ei = torch.stack([el.src.long(), el.tgt.long()])
    assert int((ei == 7).sum()) == 0
    keep = torch.ones(x.shape[0], dtype=torch.bool, device=dev)
    keep[7] = False
    ref = _ref(conv.nn, xd.masked_fill(~keep.view(-1, 1), 0.0), ei, aggr, "source_to_target", g)
    _check(got=(out, gx, grads), ref=ref, what="nan query")


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_table_and_edge_index_give_the_same_bits(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [500, 260], 32, seed=23)
    ei = dm.knn_graph(x, 16, batch, loop=False)
    conv = _conv(_lin(32, 32, seed=24), dev, aggr=aggr)
    calls = _count(monkeypatch)
    a = _run(conv, x, ei)
    b = _run(conv, x, ei.clone(), a[3])                   # a fresh tensor: not registered, the explicit CSR route
    assert calls["table"] == 1 and calls["csr"] == 1
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


@pytest.mark.parametrize("graph", ["table", "csr"])
def test_two_runs_give_identical_bits(dev, graph):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [900, 700, 300], 64, seed=25)
    ei = dm.knn_graph(x, 16, batch, loop=True)
    if graph == "csr":
        ei = ei.clone()
    for aggr in ("add", "mean"):
        conv = _conv(_lin(64, 32, seed=26), dev, aggr=aggr)
        a = _run(conv, x, ei)
        b = _run(conv, x, ei, a[3])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for n in a[2]:
            assert torch.equal(a[2][n], b[2][n]), n


def test_passthrough_returns_x(dev):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [200, 100], 32, seed=27)
    conv = _conv(_lin(32, 32, seed=28), dev, cls=dm.DynamicEdgeConv, k=8, aggr="add")
    xx = x.clone().requires_grad_(True)
    out, xp = conv.forward_with_residual_input(xx, batch)
    (out.sum() + (xp * 2).sum()).backward()
    g1 = xx.grad.clone()
    xx.grad = None
    (conv(xx, batch).sum() + (xx * 2).sum()).backward()
    torch.testing.assert_close(g1, xx.grad, rtol=1e-6, atol=1e-6)


# ---- 3. no host sync, memory --------------------------------------------------------------------------------------------------
def test_dynamic_edge_conv_mean_adds_no_host_sync(dev):
    import deepmetv2_amd as dm
    sizes = [300, 40, 260]
    counts = torch.tensor(sizes)
    x = torch.randn(sum(sizes), 32).to(dev)
    batch = torch.repeat_interleave(torch.arange(3), counts).to(dev)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(dev)
    dm.register_batch(batch, ptr, 3, max_nodes=300, min_nodes=40)
    conv = _conv(torch.nn.Linear(64, 32), dev, cls=dm.DynamicEdgeConv, k=16, aggr="mean")
    xx = x.clone().requires_grad_(True)
    conv(xx, batch).sum().backward()                    # module loads, allocator warm-up
    torch.cuda.synchronize()
    g = torch.randn(sum(sizes), 32, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = conv(xx, batch)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(xx.grad).all())


def test_memory_stays_below_a_quarter_of_the_edge_features(dev):
    """8 x 4 000 nodes, k = 32: the growth of forward + backward against a quarter of one [E, 2F] fp32 tensor."""
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [4000] * 8, 32, seed=29)
    ei = dm.knn_graph(x, 32, batch, loop=True)
    E = ei.shape[1]
    for aggr in ("add", "mean"):
        conv = _conv(_lin(32, 32, seed=30), dev, aggr=aggr)
        xx = x.detach().clone().requires_grad_(True)
        g = torch.randn(x.shape[0], 32, device=dev)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.max_memory_allocated(dev)
        conv(xx, ei).backward(g)
        torch.cuda.synchronize(dev)
        grown = torch.cuda.max_memory_allocated(dev) - base
        assert grown < E * 64 * 4 / 4, (aggr, grown, E * 64)
        assert bool(torch.isfinite(xx.grad).all())


# ---- 4. unchanged behaviour -----------------------------------------------------------------------------------------------------
def test_other_requests_keep_their_routes(dev, monkeypatch):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [200, 100], 32, seed=31)
    ei = dm.knn_graph(x, 8, batch, loop=True)
    nn = _lin(32, 32, seed=32)
    calls = _count(monkeypatch)
    _conv(nn, dev, aggr="max")(x, ei)
    for dt in (torch.bfloat16, torch.float16):
        with torch.autocast("cuda", dtype=dt):
            _conv(nn, dev, aggr="add")(x, ei)
        c = _conv(nn, dev, aggr="mean")
        c.compute_dtype = dt
        c(x, ei)
    assert calls["table"] == 0 and calls["csr"] == 0
    before = calls["edge_features"]
    c = _conv(torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Identity()), dev, aggr="add")
    c(x, ei)
    assert calls["table"] == 0 and calls["csr"] == 0 and calls["edge_features"] == before + 1


@pytest.mark.parametrize("aggr", ["add", "sum", "mean"])
def test_switch_restores_the_generic_route(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [300, 70], 64, seed=33)
    ei = dm.knn_graph(x, 12, batch, loop=True)
    monkeypatch.setenv(SWITCH, "0")
    calls = _count(monkeypatch)
    nn = _lin(64, 32, seed=34)
    got = _run(_conv(nn, dev, aggr=aggr), x, ei)
    assert calls["table"] == 0 and calls["csr"] == 0 and calls["edge_features"] == 1
    _check(got, _ref(nn, x, ei, aggr, "source_to_target", got[3]), "generic")


# ---- 5. full size ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_full_size_dynamic_edge_conv(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    x, batch = _knn_inputs(dev, [4500] * 64, 32, seed=35)
    ei = dm.knn_graph(x, 16, batch, loop=True)
    _parity(dev, _lin(32, 32, seed=36), x, batch, ei, aggr, monkeypatch=monkeypatch, form="table",
            cls=dm.DynamicEdgeConv, on_device=True, k=16)

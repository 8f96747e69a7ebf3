"""Every EdgeConv route on kNN tables with SHORT rows, against a float64 reference.

A kNN table with self loops over events of at least k nodes is built expecting full rows (`full_rows`: its [2,E] view is
sized N k without asking the device).  Some rows still come out short: a query with a NaN or +-inf coordinate finds
nobody, and a node more than ~1e5 from every other node of its event keeps only itself (the kernels' 1e10 squared-
distance sentinel).  Upstream (torch_cluster.knn, oracle.ref_ops.knn_graph) drops those slots: a short row is fewer
edges.  Here every route -- fused Linear-max fp32 / bf16, the bf16 table kernel (_EdgeMLP2Bf16), the fused edge-list
routes (_EdgeMLP2F32, _EdgeMLP2Bf16Edges) and the generic route -- runs through DynamicEdgeConv, EdgeConv over
knn_graph(loop=True) and EdgeConv over knn_table, and is held to ref_ops.edge_conv in float64 over the oracle's edges,
with exact checks on the short rows: 0 for an empty row (R3), the single message for a row that holds only its node
(also under mean), finite gradients, and the same bits as an explicit edge_index of the same edges."""
import copy

import pytest
import torch

import edge_mlp_reference as ref

pytestmark = pytest.mark.gpu

SIZES = [300, 40, 17]
K = 16
FAR = 2e5               # (2e5)^2 = 4e10 > the 1e10 sentinel: never a neighbour
SHORT_CASES = ["nan_query", "inf_query", "far_outlier", "far_event"]
CASES = SHORT_CASES + ["control"]


# ---- graph cases ---------------------------------------------------------------------------------------------------------
def _case(name, D, seed=0, sizes=SIZES, k=K):
    """(coords [N,D] float32 CPU, batch [N] int64 CPU): every event holds >= k nodes, so the table has `full_rows`."""
    sizes = list(sizes) + ([k] if name == "far_event" else [])
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor(sizes, dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    x = torch.randn(int(counts.sum()), D, generator=g)
    ptr = [0] + counts.cumsum(0).tolist()
    if name == "nan_query":         # first and last node of an event, and the last node of the batch
        x[ptr[0], 1 % D] = float("nan")
        x[ptr[1] - 1, 0] = float("nan")
        x[ptr[-1] - 1, D - 1] = float("nan")
    elif name == "inf_query":
        x[ptr[0] + 5, 0] = float("inf")
        x[ptr[1] + 3, D - 1] = float("-inf")
    elif name == "far_outlier":     # its row holds only itself, and nobody picks it
        x[ptr[1] + 7, 0] += FAR
    elif name == "far_event":       # an event of exactly k nodes, FAR apart: every row in it holds one entry
        lo = ptr[-2]
        x[lo:, :] = 0.0
        x[lo:, 0] = torch.arange(k, dtype=torch.float32) * FAR
    return x, batch


def _ref_edges(coords, batch, k=K):
    """the oracle's kNN graph, source -> target, grouped by target in (d, j) order; and in / out degrees"""
    from oracle import ref_ops
    ei = ref_ops.knn_graph(coords, k, batch, loop=True)
    N = coords.shape[0]
    return ei, torch.bincount(ei[1], minlength=N), torch.bincount(ei[0], minlength=N)


def _check_rows(table, coords, batch, k=K):
    ei, _, _ = _ref_edges(coords, batch, k)
    assert table.full_rows
    edges = table.edge_list()
    assert int(edges.rowptr[-1]) == edges.src.numel() == edges.tgt.numel() == edges.num_edges == ei.shape[1]
    assert int(edges.src.min()) >= 0
    assert torch.equal(edges.src.long().cpu(), ei[0]) and torch.equal(edges.tgt.long().cpu(), ei[1])
    return ei


# ---- 1. edge-list invariants: only the kNN and table_edges kernels run here ------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_knn_table_edge_list_is_the_oracles(dev, case):
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()                      # nothing pending from earlier tests
    coords, batch = _case(case, 3, seed=1)
    cd, bd = coords.to(dev), batch.to(dev)
    ei = _check_rows(dm.knn_table(cd, K, bd), coords, batch)
    assert (ei.shape[1] < coords.shape[0] * K) == (case != "control")
    # the [2,E] view handed to the caller stays sized N k (no device read) and is checked later: -1 where a row is short;
    # torch_cluster.knn's self-query form hands out the same view and posts the same check
    for view, row in ((lambda: dm.knn_graph(cd, K, bd, loop=True), 0),
                      (lambda: dm.knn_graph(cd, K, bd, loop=True, flow="target_to_source"), 1),
                      (lambda: dm.knn(cd, cd, K, bd, bd), 1)):
        v = view()
        assert v.shape == (2, coords.shape[0] * K)
        assert int((v[row].cpu() < 0).sum()) == coords.shape[0] * K - ei.shape[1]
        if case == "control":
            dm.raise_deferred_errors()
        else:
            with pytest.raises(RuntimeError, match="came out short"):
                dm.raise_deferred_errors()
            dm.raise_deferred_errors()              # every check reported once


def test_knn_short_row_posts_deferred_check(dev):
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()
    coords, batch = _case("nan_query", 3, seed=2)
    cd, bd = coords.to(dev), batch.to(dev)
    dm.knn(cd, cd, K, bd, bd)
    with pytest.raises(RuntimeError, match="knn: a neighbour row came out short"):
        dm.raise_deferred_errors()
    _check_rows(dm.knn_table(cd, K, None), coords, torch.zeros(coords.shape[0], dtype=torch.int64))


# ---- 2. every route, every entry, against float64 ---------------------------------------------------------------------------
def _mlp(Hin, H1, H2, act2, bn, seed):
    torch.manual_seed(seed)
    mods = [torch.nn.Linear(2 * Hin, H1), torch.nn.ELU(), torch.nn.Linear(H1, H2)]
    if act2:
        mods.append(torch.nn.ELU())
    if bn is not None:
        b = torch.nn.BatchNorm1d(H2)
        with torch.no_grad():
            b.weight.uniform_(0.5, 1.5)
            b.weight[::3].neg_()
            b.bias.uniform_(-0.5, 0.5)
            b.running_mean.uniform_(-0.2, 0.2)
            b.running_var.uniform_(0.5, 1.5)
        b.train(bn == "train")
        mods.append(b)
    return torch.nn.Sequential(*mods)


# route -> (native entries that prove the route ran, nn kind, (Hin, H1, H2), aggregations, BatchNorm modes, bf16 request,
#           environment, edge-list route: the table and an explicit edge_index must give the same bits)
ROUTES = {
    "linear_max_f32": (("gather_max",), "linear", (32, 0, 32), ["max"], [None], None, {}, False),
    "linear_max_f32_h64": (("gather_max",), "linear", (64, 0, 64), ["max"], [None], None, {}, False),
    "linear_max_bf16": (("gather_max_bf16q",), "linear", (32, 0, 32), ["max"], [None], "compute", {}, False),
    "mlp2_bf16_table": (("edge_mlp2_bf16", "edge_mlp2_bn_bf16"), "mlp", (32, 48, 32), ["max", "add"], [None, "train", "eval"], "autocast", {},
                        False),
    "mlp_f32": (("edge_mlp_fwd_f32",), "mlp", (16, 24, 16), ["max", "add", "mean"], [None, "train", "eval"], None, {}, True),
    "mlp_bf16_edges_mean": (("edge_mlp_fwd_bf16",), "mlp", (32, 48, 32), ["mean"], [None, "train", "eval"], "compute", {},
                            True),
    "mlp_bf16_edges_width": (("edge_mlp_fwd_bf16",), "mlp", (16, 32, 32), ["max", "add", "mean"], [None, "train", "eval"],
                             "compute", {}, True),
    "generic_switch": (("edge_features",), "mlp", (16, 24, 16), ["max", "add", "mean"], [None, "train", "eval"], None,
                       {"DMET_EDGE_MLP_F32": "0"}, True),
    "generic_nn": (("edge_features",), "relu", (16, 24, 8), ["max", "add", "mean"], [None], None, {}, True),
}


def _params():
    """every route x entry x applicable case (knn_graph under both flows); aggregation, BatchNorm mode and act2 cycle
    with nested periods, so that on every route each pair of aggregation, BatchNorm mode and act2 values meets"""
    out = []
    flows = ("source_to_target", "target_to_source")
    for route, (_n, _kind, _w, aggrs, bns, _bf, _env, _el) in ROUTES.items():
        i = 0
        period = len(aggrs) * len(bns)
        for entry, case, flow in ([("dynamic", c, flows[0]) for c in ("nan_query", "inf_query")]
                                  + [("knn_graph", c, f) for c in CASES for f in flows]
                                  + [("knn_table", c, flows[0]) for c in CASES]):
            aggr = aggrs[i % len(aggrs)]
            bn = bns[(i // len(aggrs)) % len(bns)]
            act2 = ((i // period) if period > 1 else i) % 2 == 0
            out.append(pytest.param(route, entry, case, aggr, bn, act2, flow,
                                    id=f"{route}-{entry}-{case}-{aggr}-{bn}-{'act2' if act2 else 'noact2'}-{flow[:3]}"))
            i += 1
    return out


def _make_nn(route, act2, bn, seed=7):
    _n, kind, (Hin, H1, H2), *_ = ROUTES[route]
    if kind == "linear":
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(2 * Hin, H2))
    if kind == "relu":
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(2 * Hin, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2))
    return _mlp(Hin, H1, H2, act2, bn, seed)


def _emulate_table(nn, x, ei, aggr, flow):
    """The bf16 table kernel's recipe (csrc/edgemlp.hip, as test_gpu_parity.py emulates it): edge features and W1 rounded
    to bf16, h1 = bf16(ELU(.)), W2 rounded to bf16, products exact, sums in float64 kept as fp32; the BatchNorm in float64.
    (out, post-BatchNorm messages [E, H2])"""
    bf = lambda t: t.to(torch.bfloat16).to(torch.float64)
    mods = list(copy.deepcopy(nn).to(x.device))
    bn = mods.pop() if isinstance(mods[-1], torch.nn.BatchNorm1d) else None
    l1, l2, act2 = mods[0], mods[2], len(mods) == 4
    tgt, src = ref.ends(ei, flow)
    N = x.shape[0]
    with torch.no_grad():
        xi = x[tgt]
        feat = torch.cat([bf(xi), bf(x[src] - xi)], dim=1)
        z1 = (feat @ bf(l1.weight).T).float() + l1.bias
        h1 = bf(torch.nn.functional.elu(z1))
        m = (h1 @ bf(l2.weight).T).float() + l2.bias
        if act2:
            m = torch.nn.functional.elu(m)
        if bn is not None:
            if bn.training:
                mean, var = m.double().mean(0), m.double().var(0, unbiased=False)
            else:
                mean, var = bn.running_mean.double(), bn.running_var.double()
            a = bn.weight.double() / torch.sqrt(var + bn.eps)
            m = (a * m.double() + (bn.bias.double() - mean * a)).float()
        idx = tgt.view(-1, 1).expand(-1, m.shape[1])
        if aggr == "max":
            out = torch.zeros((N, m.shape[1]), dtype=m.dtype, device=m.device).scatter_reduce(0, idx, m, "amax",
                                                                                               include_self=False)
        else:
            out = torch.zeros((N, m.shape[1]), dtype=m.dtype, device=m.device).index_add_(0, tgt, m)
    return out, m


def _conv(cls, nn, dev, **kw):
    """an operator over a copy of nn with nn's weights and statistics (the constructors reset nn, as PyG's do)"""
    conv = cls(copy.deepcopy(nn), **kw)
    conv.nn.load_state_dict(nn.state_dict())
    return conv.to(dev)


def _run(conv, x, graph, g, bf16, batch=None):
    """forward (+ autocast when asked) and backward: (out, gx, {param: grad}, {buffer: value})"""
    import deepmetv2_amd as dm
    conv.zero_grad(set_to_none=True)
    if bf16 == "compute":
        conv.compute_dtype = torch.bfloat16
    xx = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16 == "autocast"):
        out = conv(xx, batch) if isinstance(conv, dm.DynamicEdgeConv) else conv(xx, graph)
    out.backward(g)
    grads = {n: p.grad.detach().clone() for n, p in conv.nn.named_parameters() if p.grad is not None}
    bufs = {n: b.detach().clone() for n, b in conv.nn.named_buffers()}
    return out.detach(), xx.grad.detach().clone(), grads, bufs


def _ref(nn, x, ei, aggr, g):
    """float64 reference over the oracle's edges: (out, gx, grads, buffers, messages [E, F_out])"""
    from oracle import ref_ops
    nn64 = copy.deepcopy(nn).double()
    msg_nn = copy.deepcopy(nn64)
    xx = x.detach().cpu().double().requires_grad_(True)
    out = ref_ops.edge_conv(xx, ei, nn64, aggr)
    out.backward(g.cpu().double())
    with torch.no_grad():               # the same messages again (a training-mode norm sees the same batch)
        xd = xx.detach()
        msg = msg_nn(torch.cat([xd[ei[1]], xd[ei[0]] - xd[ei[1]]], dim=1))
    grads = {n: p.grad.detach() for n, p in nn64.named_parameters() if p.grad is not None}
    bufs = {n: b.detach() for n, b in nn64.named_buffers()}
    return out.detach(), xx.grad.detach(), grads, bufs, msg


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _within(a, b, rel, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, scale = _amax(a - b), max(_amax(b), 1e-6)
    assert err <= rel * scale, (what, err, scale)


def _layer_scales(grads):
    scale = {}
    for n, gr in grads.items():
        layer = n.rsplit(".", 1)[0]
        scale[layer] = max(scale.get(layer, 0.0), _amax(gr))
    return scale


def _counter(monkeypatch, names):
    """a list that receives the result of every call of the _native entries `names`"""
    from deepmetv2_amd import _native
    calls = []

    def wrap(real):
        def call(*a, **k):
            res = real(*a, **k)
            calls.append(res)
            return res
        return call
    for name in names:
        monkeypatch.setattr(_native, name, wrap(getattr(_native, name)))
    return calls


def _check_route(dev, monkeypatch, route, entry, case, aggr, bn, act2, flow, sizes=SIZES, seed=0):
    import deepmetv2_amd as dm
    native, kind, (Hin, _H1, H2), _a, _b, bf16, env, edge_route = ROUTES[route]
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    try:                                            # a check left pending by an earlier test that failed early
        dm.raise_deferred_errors()
    except RuntimeError:
        pass
    calls = _counter(monkeypatch, native)
    nn = _make_nn(route, act2, bn)
    if entry == "dynamic":                          # the coordinates are the features
        coords, batch = _case(case, Hin, seed=seed, sizes=sizes)
        x = coords
    else:
        coords, batch = _case(case, 3, seed=seed, sizes=sizes)
        x = torch.randn(coords.shape[0], Hin, generator=torch.Generator().manual_seed(seed + 1))
    ei, indeg, outdeg = _ref_edges(coords, batch)
    N = x.shape[0]
    g = torch.randn(N, H2, generator=torch.Generator().manual_seed(seed + 2))
    xd, cd, bd, gd = x.to(dev), coords.to(dev), batch.to(dev), g.to(dev)

    if entry == "dynamic":
        conv = _conv(dm.DynamicEdgeConv, nn, dev, k=K, aggr=aggr)
        got = _run(conv, xd, None, gd, bf16, batch=None if len(sizes) == 1 else bd)
    elif entry == "knn_graph":
        conv = _conv(dm.EdgeConv, nn, dev, aggr=aggr, flow=flow)
        got = _run(conv, xd, dm.knn_graph(cd, K, bd, loop=True, flow=flow), gd, bf16)
    else:
        conv = _conv(dm.EdgeConv, nn, dev, aggr=aggr)
        table = dm.knn_table(cd, K, bd)
        assert table.full_rows
        got = _run(conv, xd, table, gd, bf16)
    assert len(calls) == 1, (route, "route not taken")
    out, gx, grads, bufs = got
    ref_out, ref_gx, ref_grads, ref_bufs, msg = _ref(nn, x, ei, aggr, g)

    # exact: finite everywhere, 0 for an empty row (R3), no gradient to a node nobody reads, one message for a row of one
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all())
    for n, gr in grads.items():
        assert bool(torch.isfinite(gr).all()), n
    empty = indeg == 0
    assert bool((out.cpu()[empty] == 0).all())
    assert bool((gx.cpu()[empty & (outdeg == 0)] == 0).all())
    assert (int(empty.sum()) > 0) == (case in ("nan_query", "inf_query"))
    first = torch.cumsum(indeg, 0) - indeg          # ei is grouped by target: row i starts at edge first[i]
    self_only = ((indeg == 1) & (ei[0][first.clamp(max=max(ei.shape[1] - 1, 0))] == torch.arange(N))).nonzero().view(-1)
    assert (self_only.numel() > 0) == (case in ("far_outlier", "far_event"))

    # against float64
    if bf16 is None:
        rel_out, rel_grad = 1e-4, 1e-4
        _within(out, ref_out, rel_out, "out")
    elif native[0] in ("edge_mlp_fwd_bf16", "edge_mlp2_bf16"):   # forward tight against the kernel's recipe
        rel_out, rel_grad = 2e-2, 2e-2
        emulate = ref.emulate if native[0] == "edge_mlp_fwd_bf16" else _emulate_table
        emu, _m = emulate(nn, xd, ei.to(dev), aggr, "source_to_target")
        _within(out, emu, 2e-3, "out vs recipe")
        _within(out, ref_out, rel_out, "out")
        if bn == "train":
            # the batch statistics behind the running ones, against the recipe's messages over the VALID edges: an
            # empty slot counted as an edge (0.3 - 4 % of the slots here) would move them by about that fraction
            pre = torch.nn.Sequential(*list(nn)[:-1])
            _e, m = emulate(pre, xd, ei.to(dev), "add", "source_to_target")
            bnm, mom = nn[-1], nn[-1].momentum
            for name, stat in (("running_mean", m.double().mean(0)), ("running_var", m.double().var(0, unbiased=True))):
                key = f"{len(nn) - 1}.{name}"          # conv.nn's buffer names carry the module's position
                got_stat = (bufs[key].double() - (1 - mom) * getattr(bnm, name).double().to(dev)) / mom
                torch.testing.assert_close(got_stat, stat, rtol=1e-3, atol=1e-4 * _amax(stat), msg=name)
    else:
        rel_out, rel_grad = 2e-2, 2e-2
        _within(out, ref_out, rel_out, "out")
    if self_only.numel():                           # the single message, not divided by k under mean
        _within(out.cpu()[self_only], msg[first[self_only]], rel_out, "row of one entry")
    # bf16 winners: gradients follow the maxima the kernel picked (a bf16 rounding may reorder two messages within 2^-8
    # of each other), so the float64 composition takes those winners
    win = None
    if native[0] == "edge_mlp_fwd_bf16" and aggr == "max":
        _g, win = ref.kernel_winners(nn, xd, ei.to(dev), "source_to_target")
    elif native[0] == "gather_max_bf16q":
        slot = calls[0][1].long().cpu()             # winning slot per (node, channel), 255: none; valid slots come first
        win = torch.where(slot == 255, torch.full_like(slot, -1), first.view(-1, 1) + slot).to(dev)
    if win is not None:
        _o, ref_gx, ref_grads = ref.ref64(nn, xd, ei.to(dev), aggr, "source_to_target", gd, win)
    _within(gx, ref_gx, rel_grad, "gx")
    assert grads.keys() == ref_grads.keys()
    scale = _layer_scales(ref_grads)
    for n in ref_grads:
        err = _amax(grads[n].cpu().double() - ref_grads[n].cpu().double())
        tol = rel_grad * max(scale[n.rsplit(".", 1)[0]], 1e-6)
        assert err <= tol, (n, err, tol)
    for n, b in ref_bufs.items():                   # running statistics over the VALID edges (unbiased variance: E - 1)
        if b.dtype == torch.int64:
            assert torch.equal(bufs[n].cpu(), b), n
        elif bf16 is None:
            torch.testing.assert_close(bufs[n].cpu().double(), b, rtol=1e-5, atol=1e-6, msg=n)
        else:
            torch.testing.assert_close(bufs[n].cpu().double(), b, rtol=3e-2, atol=2e-3, msg=n)

    # the sync-free [2,E] view was handed out: a short row is reported by the deferred check, at the latest here
    if entry == "knn_graph" and case != "control":
        with pytest.raises(RuntimeError, match="came out short"):
            dm.raise_deferred_errors()
    dm.raise_deferred_errors()

    # the same compacted edges as an explicit edge_index: the same bits on the edge-list routes
    if edge_route:
        eflow = flow if entry == "knn_graph" else "source_to_target"
        explicit = (ei if eflow == "source_to_target" else ei.flip(0)).to(dev)
        conv2 = _conv(dm.EdgeConv, nn, dev, aggr=aggr, flow=eflow)
        n_calls = len(calls)
        again = _run(conv2, xd, explicit, gd, bf16)
        assert len(calls) == n_calls + 1, (route, "explicit edge_index took another route")
        assert torch.equal(again[0], out) and torch.equal(again[1], gx)
        for n in grads:
            assert torch.equal(again[2][n], grads[n]), n
        for n in bufs:
            assert torch.equal(again[3][n], bufs[n]), n


@pytest.mark.parametrize("route,entry,case,aggr,bn,act2,flow", _params())
def test_route_on_short_rows(dev, monkeypatch, route, entry, case, aggr, bn, act2, flow):
    _check_route(dev, monkeypatch, route, entry, case, aggr, bn, act2, flow)


@pytest.mark.parametrize("case,aggr,bn", [("far_outlier", "mean", "train"), ("nan_query", "max", "eval"),
                                          ("control", "add", None)])
def test_mlp_f32_large_events(dev, monkeypatch, case, aggr, bn):
    """two events of 4 500 nodes (the DRN's event size) on the fp32 edge-list route"""
    _check_route(dev, monkeypatch, "mlp_f32", "knn_table", case, aggr, bn, True, "source_to_target",
                 sizes=[4500, 4500], seed=3)


@pytest.mark.parametrize("route", ["linear_max_f32", "linear_max_f32_h64", "linear_max_bf16", "mlp_f32", "mlp_bf16_edges_mean",
                                   "mlp_bf16_edges_width", "generic_nn"])
def test_dynamic_edge_conv_without_batch(dev, monkeypatch, route):
    """batch=None counts as one full event: the table has `full_rows` there too"""
    _check_route(dev, monkeypatch, route, "dynamic", "nan_query", ROUTES[route][3][-1], None, True, "source_to_target",
                 sizes=[200])


"""multi_aggregate, scatter_std, DegreeScalerAggregation and PNAConv on the GPU (csrc/multi_aggr.hip,
deepmetv2_amd/pna.py) against the float64 restatements of tests/pna_reference.py on the inputs of tests/pna_cases.py.

Bounds per element, u = 2^-24, n the row length, mean|x| and var the reference's:
  count, min, max and their positions: equal      sum: (n + 2) u sum|x|      mean: (n + 3) u mean|x|
  var: (2n + 8) u var + ((n + 2) u mean|x|)^2 + 1e-45      std (var > 4e-5): var_bound / (2 std) + 2 u std
  g_x: pna_reference.grad_bound, derived there from the kernels' chain: (n_j + 12) u times the summed magnitudes of the
       terms of the source's n_j positions, plus the propagated errors of the mean and of the standard deviation.
tests/test_pna_host.py holds an fp32 emulation of the kernels' chains under half of each of them on these inputs.
Every row and every element is checked; each check prints its largest error / bound ratio before it asserts.
"""
import pytest
import torch

import pna_cases as pc
import pna_reference as pr
import poisoned_alloc as pa

pytestmark = pytest.mark.gpu

ALL = pr.KINDS
PNA4 = ("mean", "min", "max", "std")


def _graph(graph, Nt, Ns, dev, bipartite=False):
    from deepmetv2_amd.graph import BipartiteTable, EdgeList, NeighborTable
    if "nbr" in graph:
        nbr = graph["nbr"].to(dev)
        return BipartiteTable(nbr, None, None, Ns) if bipartite else NeighborTable(nbr, None, dense=False)
    src, rowptr = graph["src"].to(dev), graph["rowptr"].to(dev)
    tgt = torch.repeat_interleave(torch.arange(Nt, dtype=torch.int32, device=dev), rowptr.diff().long())
    return EdgeList(src, tgt, rowptr, Nt, num_src=Ns)


def _run(x, graph, aggrs, groups, g_out):
    import deepmetv2_amd as dm
    xx = x.detach().requires_grad_(True)        # shares x's storage: an unaligned view stays one
    out, count = dm.multi_aggregate(xx, graph, aggrs, groups)
    out.backward(g_out.view_as(out))
    return out.detach(), count, xx.grad


def _ratio(name, what, err, lim):
    r = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: {name} max err/bound {r:.3f}")
    assert bool((err <= lim).all()), (what, name, r)


def _check(case, aggrs, groups, dev, bipartite=False, what=""):
    x, graph, pos, Nt, ref = case
    F = x.shape[1]
    assert pr.clamp_is_clear(ref), what        # the condition on the inputs, asserted on the reference
    g_out = pc.upstream_gradient(aggrs, Nt, F, groups, len(what))
    out, count, g_x = _run(x.to(dev), _graph(graph, Nt, x.shape[0], dev, bipartite), aggrs, groups, g_out.to(dev))
    assert out.shape == ((Nt, len(aggrs), F) if groups == 1 else (Nt, groups, len(aggrs), F // groups)), what
    assert count.dtype == torch.int32 and torch.equal(count.cpu().long(), ref["count"]), what
    # the positions the backward is given: the wrapper's own saved rows, the reference's positions exactly
    from deepmetv2_amd import _native
    idx, rowptr = (graph["nbr"], None) if "nbr" in graph else (graph["src"], graph["rowptr"])
    raw, _cnt, (_mean, _var, amin, amax) = _native._multi_aggr_fwd(x.to(dev), idx.to(dev), None if rowptr is None else rowptr.to(dev),
                                                                  Nt, aggrs, groups)
    assert torch.equal(raw.view_as(out), out), what
    for name, arg in (("argmin", amin), ("argmax", amax)):
        assert (arg is not None) == (name[3:] in aggrs), (what, name)
        if arg is not None:
            assert arg.dtype == torch.int32 and torch.equal(arg.cpu().long(), ref[name]), (what, name)
    got = pr.layout(out.cpu().double(), aggrs, groups)
    b = pr.bounds(ref)
    empty = ref["count"] == 0
    for a in aggrs:
        assert bool(torch.isfinite(got[a]).all()) and bool((got[a][empty] == 0).all()), (what, a)
        if a in ("min", "max"):
            assert torch.equal(got[a], ref[a]), (what, a)
        elif a == "std":
            big = ref["var"] > 4e-5
            assert bool((got[a][~big] == 0).all()), (what, "std below the clamp")
            _ratio(a, what, (got[a] - ref[a]).abs()[big], b[a][big])
        else:
            _ratio(a, what, (got[a] - ref[a]).abs(), b[a])
    g64 = pr.layout(g_out.double(), aggrs, groups)
    want, n_j = pr.grad(x, *pos, ref, g64)
    gx = g_x.cpu().double()
    assert gx.shape == want.shape and bool(torch.isfinite(gx).all()), what
    _ratio("g_x", what, (gx - want).abs(), pr.grad_bound(x, *pos, ref, g64))
    assert bool((gx[n_j == 0] == 0).all()), what          # a source nobody lists
    return got, gx, ref


# ---- 1. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 16, 17, 64])
@pytest.mark.parametrize("F,groups", [(5, 1), (64, 4)])
def test_table_widths(dev, k, F, groups):
    _got, _gx, ref = _check(pc.case("table", F, "normal", 20 + k, k=k), ALL, groups, dev, what=f"table k={k} F={F}")
    assert bool((ref["count"] == 0).any()) and int(ref["count"].max()) <= k


@pytest.mark.parametrize("F,groups", [(1, 1), (3, 1), (4, 1), (4, 4), (5, 1), (64, 1), (65, 1), (256, 1), (256, 4)])
def test_feature_widths(dev, F, groups):
    _check(pc.case("table", F, "normal", 30, k=3), ALL, groups, dev, what=f"table F={F} G={groups}")
    _check(pc.case("list", F, "normal", 31), PNA4, groups, dev, what=f"list F={F} G={groups}")


@pytest.mark.parametrize("aggrs", [("sum",), ("max", "min"), ("var",), ("std", "sum"), ("mean", "var")])
def test_subsets_in_request_order(dev, aggrs):
    _check(pc.case("table", 8, "normal", 32, k=17), aggrs, 2, dev, what=f"subset {aggrs}")


def test_bipartite_table(dev):
    case = pc.case("table", 12, "normal", 33, k=16, num_src=57)
    assert case[0].shape[0] == 57 and case[3] == sum(pc.SIZES)
    _check(case, ALL, 1, dev, bipartite=True, what="bipartite")


def test_edge_list_degrees(dev):
    case = pc.case("list", 5, "normal", 34)
    _got, _gx, ref = _check(case, ALL, 1, dev, what="list")
    assert {0, 1, 2, 63, 64, 65, 300} <= set(ref["count"].tolist())


def test_ungrouped_edge_index_tensor(dev):
    """A shuffled [2, E] tensor through PNAConv's own resolution: grouped internally, results in the caller's node order."""
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import edge_list_from_edge_index
    x, graph, pos, Nt, ref = pc.case("list", 5, "normal", 34)
    tgt, src, _valid = pos
    perm = torch.randperm(tgt.numel(), generator=torch.Generator().manual_seed(35))
    ei = torch.stack([src[perm], tgt[perm]]).to(dev)
    edges = edge_list_from_edge_index(ei, Nt, "source_to_target")
    assert edges.perm is not None
    out, count = dm.multi_aggregate(x.to(dev), edges, ("sum", "mean", "min", "max", "var"))
    got = pr.layout(out.cpu().double(), ("sum", "mean", "min", "max", "var"), 1)
    assert torch.equal(count.cpu().long(), ref["count"])
    assert torch.equal(got["min"], ref["min"]) and torch.equal(got["max"], ref["max"])
    b = pr.bounds(ref)
    for a in ("sum", "mean", "var"):          # another (stable) order inside a row: the same bounds
        _ratio(a, "ungrouped", (got[a] - ref[a]).abs(), b[a])


# ---- 2. data regimes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,F,data,k", [("table", 8, "offset1000", 16), ("table", 5, "offset1000", 3), ("list", 4, "offset1000", 3),
                                           ("table", 8, "offset-50", 64), ("list", 5, "offset-50", 3)])
def test_cancellation_regimes(dev, kind, F, data, k):
    """An offset much larger than the spread: a variance formed from two fp32 means is thousands of bounds away here."""
    _got, _gx, ref = _check(pc.case(kind, F, data, 40, k=k), ALL, 1, dev, what=f"{kind} {data}")
    long = ref["count"] > 1
    assert bool((ref["var"][long] < 0.01 * ref["mean"][long] ** 2).all())


@pytest.mark.parametrize("kind,k", [("table", 3), ("table", 17), ("list", 3)])
def test_small_integers_are_exact(dev, kind, k):
    got, _gx, ref = _check(pc.case(kind, 6, "ints", 41, k=k), ALL, 2, dev, what=f"{kind} ints")
    assert torch.equal(got["sum"], ref["sum"])
    assert int(ref["count"].max()) > 1


def test_rows_of_one_repeated_value(dev):
    """var and std exactly 0, the positions the row's lowest valid slot, the whole min / max gradient on that slot."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    case = pc.case("table", 6, "const_rows", 42, k=16)
    x, graph, (tgt, src, valid), Nt, ref = case
    got, gx, _ref = _check(case, ALL, 1, dev, what="const rows")
    assert bool((got["var"] == 0).all()) and bool((got["std"] == 0).all())
    _out, _count, (_mean, _var, amin, amax) = _native._multi_aggr_fwd(x.to(dev), graph["nbr"].to(dev), None, Nt, ALL, 1)
    pos = torch.nonzero(valid).view(-1)
    first = torch.full((Nt,), -1, dtype=torch.long).scatter_reduce_(0, tgt[pos], pos, "amin", include_self=False)
    first = torch.where(ref["count"] > 0, first, torch.full_like(first, -1))
    assert torch.equal(amin.cpu().long(), first.view(-1, 1).expand(Nt, 6))
    assert torch.equal(amax.cpu().long(), first.view(-1, 1).expand(Nt, 6))
    # only min and max requested: g_x[j] is the sum of the gradients of the rows whose first valid slot holds j
    g = pc.upstream_gradient(("min", "max"), Nt, 6, 1, 43)
    xx = x.to(dev).requires_grad_(True)
    out, _c = dm.multi_aggregate(xx, _graph(graph, Nt, Nt, dev), ("min", "max"))
    out.backward(g.to(dev).view_as(out))
    rows = torch.nonzero(first >= 0).view(-1)
    want = torch.zeros(Nt, 6, dtype=torch.float64).index_add_(0, src[first[rows]], (g[rows, 0, 0] + g[rows, 0, 1]).double())
    mag = torch.zeros(Nt, 6, dtype=torch.float64).index_add_(0, src[first[rows]], (g[rows, 0, 0].abs() + g[rows, 0, 1].abs()).double())
    n_j = torch.bincount(src[pos], minlength=Nt).double().view(-1, 1)
    assert bool(((xx.grad.cpu().double() - want).abs() <= (n_j + 12) * pr.U * mag).all())


# ---- 3. properties ---------------------------------------------------------------------------------------------------------
def test_unaligned_view_gives_the_same_bits(dev):
    x, graph, _pos, Nt, _ref = pc.case("table", 64, "normal", 50, k=17)
    x = x.to(dev)
    flat = torch.zeros(x.numel() + 1, device=dev)
    view = flat[1:].view_as(x)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and x.data_ptr() % 16 == 0
    g = pc.upstream_gradient(ALL, Nt, 64, 4, 50).to(dev)
    gr = _graph(graph, Nt, Nt, dev)
    a, b = _run(x, gr, ALL, 4, g), _run(view, gr, ALL, 4, g)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


def test_two_runs_give_identical_bits(dev):
    x, graph, _pos, Nt, _ref = pc.case("list", 64, "normal", 51)
    g = pc.upstream_gradient(ALL, Nt, 64, 1, 51).to(dev)
    gr = _graph(graph, Nt, Nt, dev)
    a, b = _run(x.to(dev), gr, ALL, 1, g), _run(x.to(dev), gr, ALL, 1, g)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


@pytest.mark.parametrize("kind,aggrs", [("table", ALL), ("list", ALL), ("table", ("sum", "max"))])
def test_bits_do_not_depend_on_what_the_buffers_held(dev, kind, aggrs):
    """Outputs, saved rows and the backward's work rows allocated over 0xFF bytes and over 3e38 / zero bytes: the same bits,
    so every element is written and no word is read before it is."""
    from deepmetv2_amd import _native
    x, graph, _pos, Nt, _ref = pc.case(kind, 12, "normal", 52, k=17)
    x = x.to(dev)
    gr = _graph(graph, Nt, Nt, dev)
    g = pc.upstream_gradient(aggrs, Nt, 12, 2, 52).to(dev)
    table = kind == "table"
    idx, rowptr, tgt = (gr.nbr, None, None) if table else (gr.src, gr.rowptr, gr.tgt)
    rev_ptr, rev_pos = gr.reverse() if table else gr.by_source()

    def call():
        out, count, saved = _native._multi_aggr_fwd(x, idx, rowptr, Nt, aggrs, 2)
        g_x = _native._multi_aggr_bwd(g, x, count, saved, rev_ptr, rev_pos, tgt, gr.k if table else None, aggrs, 2)
        return out, count, [t for t in saved if t is not None], g_x

    got = pa.run_both(call)
    assert len(got["ones"]) == len(got["zeros_huge"]) >= 3
    for a, b in zip(got["ones"], got["zeros_huge"]):
        assert pa.differing(a, b).numel() == 0
        assert not a.is_floating_point() or bool(torch.isfinite(a).all())


def test_no_host_sync(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import NeighborTable
    x, graph, _pos, Nt, _ref = pc.case("table", 64, "normal", 53, k=16)
    x, nbr = x.to(dev), graph["nbr"].to(dev)
    g = pc.upstream_gradient(PNA4, Nt, 64, 4, 53).to(dev)
    _run(x, NeighborTable(nbr, None, dense=False), PNA4, 4, g)          # module loads, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, _count, g_x = _run(x, NeighborTable(nbr, None, dense=False), PNA4, 4, g)       # a fresh table: its reverse index too
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out).all()) and bool(g_x.abs().sum() > 0)


def test_bf16(dev):
    import deepmetv2_amd as dm
    x, graph, _pos, Nt, _ref = pc.case("table", 64, "normal", 54, k=16)
    gr = _graph(graph, Nt, Nt, dev)
    xb = x.to(dev).to(torch.bfloat16)
    out, count = dm.multi_aggregate(xb, gr, PNA4, 4)
    full, count32 = dm.multi_aggregate(xb.float(), gr, PNA4, 4)
    assert out.dtype == torch.bfloat16 and full.dtype == torch.float32 and torch.equal(out, full.to(torch.bfloat16))
    assert torch.equal(count, count32)
    xx = xb.clone().requires_grad_(True)
    dm.multi_aggregate(xx, gr, PNA4, 4)[0].float().sum().backward()
    assert xx.grad.dtype == torch.bfloat16 and bool(torch.isfinite(xx.grad.float()).all())
    with pytest.raises(TypeError):
        dm.multi_aggregate(x.to(dev).half(), gr, PNA4)              # fp16 outside fp16 autocast stays an error


# ---- 4. scatter_std and DegreeScalerAggregation ------------------------------------------------------------------------------
@pytest.mark.parametrize("unbiased", [True, False])
def test_scatter_std(dev, unbiased):
    """An unsorted index, a row of length 1, an empty row; 1000 + N(0,1).  Bound: the variance's, carried through
    sqrt(n var / c): relative var_bound / (2 var) plus 3 u for the product, the division and the square root."""
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(60)
    E, F, n = 500, 5, 9
    index = torch.randint(0, n - 2, (E,), generator=g)
    index[7] = n - 1                               # a row of length 1; row n - 2 stays empty
    x = 1000.0 + torch.randn(E, F, generator=g)
    order = torch.sort(index, stable=True).indices
    tgt, src, valid = index[order], order, torch.ones(E, dtype=torch.bool)
    ref = pr.stats(x, tgt, src, valid, n)
    assert pr.clamp_is_clear(ref) and ref["count"].tolist()[-2:] == [0, 1]
    cnt = ref["count"].double().view(-1, 1)
    denom = ((cnt - 1).clamp(min=1) if unbiased else cnt) + 1e-6
    want = (cnt * ref["var"] / denom).sqrt()
    xx = x.to(dev).requires_grad_(True)
    got = dm.scatter_std(xx, index.to(dev), dim=0, dim_size=n, unbiased=unbiased)
    assert got.shape == (n, F) and bool((got[-2:] == 0).all())
    lim = want * (pr.bounds(ref)["var"] / (2 * ref["var"].clamp(min=1e-300)) + 3 * pr.U) + 1e-45
    _ratio("std", f"scatter_std unbiased={unbiased}", (got.detach().cpu().double() - want).abs(), lim)
    got.sum().backward()          # rows of 0 and 1 entries have zero variance: the gradient there is infinite or NaN, as upstream
    keep = (index < n - 2).to(dev)
    assert bool(torch.isfinite(xx.grad[keep]).all()) and bool(xx.grad[keep].abs().sum() > 0)
    one = dm.scatter_std(x[:, 0].to(dev), index.to(dev), dim_size=n, unbiased=unbiased)       # the 1-D call shape
    assert one.shape == (n,) and torch.equal(one, got.detach()[:, 0])


def test_degree_scaler_aggregation(dev):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(61)
    E, F, n = 400, 6, 12
    index = torch.randint(0, n - 1, (E,), generator=g)
    x = torch.randn(E, F, generator=g)
    deg = torch.bincount(torch.bincount(index, minlength=n))
    scalers = ["identity", "amplification", "attenuation", "linear", "inverse_linear"]
    mod = dm.DegreeScalerAggregation(["mean", "min", "max", "std", "sum", "var"], scalers, deg).to(dev)
    xx = x.to(dev).requires_grad_(True)
    got = mod(xx, index.to(dev), dim_size=n)
    x64 = x.double().requires_grad_(True)
    want = pr.upstream_degree_scaler(x64, index, n, mod.aggr, scalers, *pr.avg_degrees(deg))
    assert got.shape == want.shape == (n, 5 * 6 * F) and bool((got[n - 1] == 0).all())
    w = torch.randn(want.shape, generator=g)
    (got * w.to(dev)).sum().backward()
    (want * w.double()).sum().backward()
    for name, a, b in (("out", got.detach(), want.detach()), ("g_x", xx.grad, x64.grad)):
        err = float((a.cpu().double() - b).abs().max() / b.abs().max())
        print(f"DegreeScalerAggregation {name}: max-norm relative error {err:.2e}")
        # every statistic of a row of n <= 60 entries is within (n + 3) u of the row's magnitude sum (the bounds above), the
        # factors add a few u, and the tensor's max-abs is of the size of the largest magnitude sum: under 4 * 64 u of it
        assert err <= 256 * pr.U
    grouped = mod(x[torch.sort(index, stable=True).indices].to(dev),
                  ptr=torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(index, minlength=n).cumsum(0)]).to(dev))
    assert torch.equal(grouped, got.detach())          # ptr: the same rows in the same order, no grouping


# ---- 5. PNAConv ------------------------------------------------------------------------------------------------------------
def _random_graph(N, E, seed):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randint(0, N - 6, (E,), generator=g)             # the last six nodes have no incoming edge
    src = torch.randint(0, N, (E,), generator=g)
    return torch.stack([src, tgt])


def _tensors(mod, x, ei, g):
    xx = x.clone().requires_grad_(True)
    out = mod(xx, ei)
    out.backward(g.to(out.dtype))
    return [("out", out.detach()), ("g_x", xx.grad)] + [(n, p.grad) for n, p in mod.named_parameters()]


def _pna_case(dev, aggrs, kwargs, env=None, monkeypatch=None, seed=70):
    """The layer on the GPU against the float64 restatement.  Tolerance per tensor, in max-norm relative to the reference
    tensor's max-abs: 8 times the error the same formula evaluated by torch in fp32 on the CPU shows against float64 on
    these inputs (the split form sums in a different but equally valid order), with a floor of 64 u."""
    import deepmetv2_amd as dm
    if env is not None:
        monkeypatch.setenv("DMET_PNA", env)
    N, C = 70, 16
    scalers = ["identity", "amplification", "attenuation"]
    ei = _random_graph(N, 400, seed)
    deg = torch.bincount(torch.bincount(ei[1], minlength=N))
    torch.manual_seed(seed)
    conv = dm.PNAConv(C, C, list(aggrs), scalers, deg, **kwargs)
    x = torch.randn(N, C, generator=torch.Generator().manual_seed(seed + 1))
    ref64 = pr.UpstreamPNAConv(C, C, list(aggrs), scalers, deg, **kwargs).double()
    ref64.load_state_dict(conv.state_dict())
    ref32 = pr.UpstreamPNAConv(C, C, list(aggrs), scalers, deg, **kwargs)
    ref32.load_state_dict(conv.state_dict())
    g = torch.randn(N, C, generator=torch.Generator().manual_seed(seed + 2))
    want = _tensors(ref64, x.double(), ei, g)
    cpu32 = _tensors(ref32, x, ei, g)
    conv = conv.to(dev)
    route = conv.route(x.to(dev))
    got = _tensors(conv, x.to(dev), ei.to(dev), g.to(dev))
    _hold(got, want, cpu32, f"{route} {kwargs}")
    return route, conv, x, ei, (want, cpu32)


def _hold(got, want, cpu32, what):
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_n, b), (_m, c) in zip(got, want, cpu32):
        scale = float(b.abs().max())
        err = float((a.cpu().double() - b).abs().max()) / scale
        base = float((c.double() - b).abs().max()) / scale
        tol = max(8 * base, 64 * pr.U)
        print(f"PNAConv {what} {name}: error {err:.2e}, fp32 torch on the CPU {base:.2e}, tolerance {tol:.2e}")
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("aggrs", [PNA4, ("sum", "var")])
@pytest.mark.parametrize("kwargs", [dict(towers=1), dict(towers=4), dict(towers=4, divide_input=True), dict(towers=1, divide_input=True)])
def test_pnaconv_fused_route(dev, aggrs, kwargs):
    route, *_ = _pna_case(dev, aggrs, kwargs)
    assert route == "fused"


def test_pnaconv_generic_route(dev):
    route, *_ = _pna_case(dev, PNA4, dict(towers=2, pre_layers=2, post_layers=2))
    assert route == "generic"


def test_pnaconv_fused_and_generic_on_the_same_weights(dev, monkeypatch):
    """The module that just ran fused, forced onto the generic route: the same float64 reference, the same tolerance."""
    r1, conv, x, ei, (want, cpu32) = _pna_case(dev, PNA4, dict(towers=4))
    monkeypatch.setenv("DMET_PNA", "0")
    assert r1 == "fused" and conv.route(x.to(dev)) == "generic"
    for p in conv.parameters():
        p.grad = None
    g = torch.randn(70, 16, generator=torch.Generator().manual_seed(72))          # _pna_case's upstream gradient
    _hold(_tensors(conv, x.to(dev), ei.to(dev), g.to(dev)), want, cpu32, "generic after fused")


def test_pnaconv_over_a_table(dev):
    """A -1-padded NeighborTable and its own edge list give the same layer output bits (the same entries in the same
    order), and isolated nodes aggregate zeros."""
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import NeighborTable
    x, graph, pos, Nt, ref = pc.case("table", 16, "normal", 73, k=16)
    deg = torch.bincount(ref["count"])
    torch.manual_seed(74)
    conv = dm.PNAConv(16, 16, list(PNA4), ["identity", "attenuation"], deg, towers=4).to(dev)
    table = NeighborTable(graph["nbr"].to(dev), None, dense=False)
    tgt, src, valid = pos
    ei = torch.stack([src[valid], tgt[valid]]).to(dev)
    a, b = conv(x.to(dev), table), conv(x.to(dev), ei)
    assert torch.equal(a, b)


def test_state_dict_names(dev):
    import deepmetv2_amd as dm
    conv = dm.PNAConv(8, 8, ["mean"], ["identity"], torch.tensor([1, 2, 3]), towers=2, train_norm=True).to(dev)
    assert sorted(conv.state_dict()) == sorted(
        ["aggr_module.avg_deg_lin", "aggr_module.avg_deg_log", "lin.weight", "lin.bias"]
        + [f"{nn}.{t}.0.{p}" for nn in ("pre_nns", "post_nns") for t in (0, 1) for p in ("weight", "bias")])
    assert {n for n, _ in conv.named_parameters()} >= {"aggr_module.avg_deg_lin", "aggr_module.avg_deg_log"}

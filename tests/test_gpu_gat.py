"""GATConv / GATv2Conv on the GPU (csrc/gat.hip, deepmetv2_amd/gat.py) against the float64 reference of
tests/gat_reference.py over the same graph.

Bars, tests/test_gpu_attention.py's.  Output, per row: |err| <= 1e-5 * bar_i + 1e-6 with bar_i = the largest |xl_j|_inf of
the row, the self entry included (the output is a convex combination of the row's xl_j).  Gradients: rtol 1e-4, atol
1e-4 * max|ref|.  The modules' outputs pass further fp32 operators and are held to the gradient bar.
tests/test_gat_host.py shows a float32 run of the reference inside half of each bar on these inputs.  One gradient needs
its scale spelt out: where every xl + xr (s_src + s_dst) of a row lies on one side of 0, where the slope is 1, and in the
large-score case (only ties at the maximum carry weight) the target-side gradient g_xr (g_s_dst) is a constant times
sum_e g_s_e, a sum that cancels exactly, and max|ref| is rounding noise; it is held to 1e-4 of the size of that sum's terms
(gat_reference.term_scale), as tests/test_gpu_attention.py does for g_q.
"""
import pytest
import torch

import attention_reference as ar
import gat_reference as gr
import poisoned_alloc as pa

pytestmark = pytest.mark.gpu
MODES = (gr.V1, gr.V2)


def _ragged(sizes, dev):
    counts = torch.tensor(sizes, dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return batch.to(dev), int(counts.sum())


def _graph(case, dev):
    """The case's graph on the GPU: a kNN table, or the grouped list of an edge index."""
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import edge_list_from_edge_index
    g = case["graph"]
    if g[0] == "knn":
        _kind, sizes, k, loop = g
        batch, N = _ragged(sizes, dev)
        return dm.knn_table(ar.coords(N, case["seed"]).to(dev), k, batch, loop=loop), N
    ei, N = gr.degree_edge_index() if g[0] == "degree" else gr.loops_edge_index()
    return edge_list_from_edge_index(ei.to(dev), N, "source_to_target"), N


def _entries(graph):
    """(tgt, src, pos or None, Ns) on the CPU of a table or an EdgeList."""
    from deepmetv2_amd.graph import EdgeList
    if isinstance(graph, EdgeList):
        return graph.tgt.cpu().long(), graph.src.cpu().long(), None, graph.num_src
    ns = graph.num_candidates if hasattr(graph, "num_candidates") else graph.num_nodes
    return gr.table_entries(graph.nbr.cpu(), ns) + (ns,)


def _op(mode):
    import deepmetv2_amd as dm
    return dm.gat_aggregate if mode == gr.V2 else dm.gat_v1_aggregate


def _run(mode, ins, graph, slope=0.2, self_loops=False, g=None, want_alpha=True):
    """GPU forward + backward of the aggregate: (out, alpha, [three gradients], g)."""
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    res = _op(mode)(*leaves, graph, negative_slope=slope, self_loops=self_loops, return_alpha=want_alpha)
    out, alpha = res if want_alpha else (res, None)
    if g is None:
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    return out.detach(), alpha, [t.grad for t in leaves], g


def _check(mode, ins, graph, slope=0.2, self_loops=False, what="", cancelling=False):
    """Output, alpha and the three gradients of the aggregate against the float64 reference over `graph`."""
    out, alpha, grads, g = _run(mode, ins, graph, slope, self_loops)
    tgt, src, pos, _ns = _entries(graph)
    Nt = out.shape[0]
    kept = (tgt != src) if self_loops else torch.ones_like(tgt, dtype=torch.bool)
    r_tgt, r_src = gr.with_self_loops(tgt, src, Nt) if self_loops else (tgt, src)
    ins64 = [t.detach().cpu().double().requires_grad_(True) for t in ins]
    r_out, r_alpha, bar = gr.run(mode, *ins64, r_tgt, r_src, slope)
    got = out.cpu()
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), what
    gr.assert_output_bar(got, r_out.detach(), bar, what)
    deg = torch.bincount(r_tgt, minlength=Nt)
    assert bool((got[deg == 0] == 0).all()), what
    # alpha over the written entries: the reference's, 0 in a skipped self loop, nothing flows back through it; without
    # the implicit entry (whose weight is not returned) rows sum to 1 within 1e-6 deg or are all 0
    assert not alpha.requires_grad
    a = alpha.cpu().double()
    if pos is not None:
        a = a.reshape(-1, a.shape[-1])
        assert bool((a[torch.ones(a.shape[0], dtype=torch.bool).index_fill(0, pos, False)] == 0).all()), what
        a = a[pos]
    r_written = torch.zeros_like(a)
    r_written[kept] = r_alpha.detach()[:int(kept.sum())]
    assert a.shape == r_written.shape, what
    torch.testing.assert_close(a, r_written, rtol=1e-4, atol=1e-6, msg=lambda m: f"{what}: alpha: {m}")
    if not self_loops:
        sums = torch.zeros((Nt, a.shape[1]), dtype=torch.float64).index_add(0, tgt, a)
        want = (deg > 0).double().view(-1, 1).expand_as(sums)
        assert bool(((sums - want).abs() <= 1e-6 * deg.clamp(min=1).view(-1, 1)).all()), (what, "alpha rows")
    r_out.backward(g.cpu().double())
    names = ("g_xl", "g_xr", "g_att") if mode == gr.V2 else ("g_xl", "g_s_src", "g_s_dst")
    target_side = "g_xr" if mode == gr.V2 else "g_s_dst"
    for name, x, ref in zip(names, grads, ins64):
        scale = None
        if cancelling and name == target_side:
            scale = gr.term_scale(mode, *[t.cpu() for t in ins], r_tgt, r_src, slope, g.cpu())
        assert x.shape == ref.grad.shape, (what, name)
        gr.assert_grad_bar(x.cpu(), ref.grad, f"{what}: {name}", scale=scale)
    return out, alpha, grads, g


# ---- 1. - 6. the aggregate on every shared case -----------------------------------------------------------------------------------------
# kNN tables with k = 1, 8, 16, 20, 33, 64 and ragged events (short rows with -1 slots, N*H on both sides of 8 and 16
# pairs per workgroup), every channel width on both sides of 16, 32 and the 16 -> 32-lane switch, in-degrees across the
# chunk boundaries 4 / 16 / 32 with a 600-entry row and a 600-entry reverse list, implicit self loops, the sign regions
# of the LeakyReLU (one sign, slope 0, slope 1, exact zeros), and scores around 100
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(gr.OPERATOR_CASES))
def test_aggregate_on_the_shared_cases(dev, name, mode):
    case = gr.OPERATOR_CASES[name]
    graph, N = _graph(case, dev)
    ins = [t.to(dev) for t in gr.inputs(mode, N, N, case["H"], case["C"], case["seed"], case["kind"])]
    out, alpha, grads, _g = _check(mode, ins, graph, case["slope"], case["self_loops"], what=f"{name}, v{mode}",
                                   cancelling=gr.cancelling(case))
    for t in [out, alpha] + grads:
        assert bool(torch.isfinite(t).all())
    if name == "knn, limits":
        assert bool((graph.nbr >= 0).all())
    if name.startswith("knn, short rows"):
        assert bool((graph.nbr[:4, 1:] < 0).any()) and bool((graph.nbr[:, 0] >= 0).all())
    if name == "self loops over knn_table(loop=False)":
        assert bool((graph.nbr[30] < 0).all())               # the one-node event: nothing but the implicit entry
        assert not bool((graph.nbr == torch.arange(N, device=dev).view(-1, 1)).any())
        assert torch.equal(out[30], ins[0][30])
    if case["kind"] == "large":
        assert float(torch.exp(torch.tensor(96.0))) == float("inf")        # what the max subtraction guards against
    if case["kind"] == "zeros":
        t = (ins[0][:, None] + ins[1][None]) if mode == gr.V2 else (ins[1][:, None] + ins[2][None])
        assert bool((t == 0).any())


# ---- 4. self loops -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_written_self_loops_do_not_matter_under_the_flag(dev, mode):
    from deepmetv2_amd.graph import edge_list_from_edge_index
    ei, N = gr.loops_edge_index()
    assert int((ei[0] == ei[1]).sum()) >= 17
    bare = ei[:, ei[0] != ei[1]]
    ins = [t.to(dev) for t in gr.inputs(mode, N, N, 3, 22, seed=82)]
    with_loops = edge_list_from_edge_index(ei.to(dev), N, "source_to_target")
    without = edge_list_from_edge_index(bare.to(dev), N, "source_to_target")
    a_out, _a, a_grads, g = _run(mode, ins, with_loops, self_loops=True)
    b_out, _b, b_grads, _g = _run(mode, ins, without, self_loops=True, g=g)
    bar = torch.full((N,), float(ins[0].abs().max()))
    gr.assert_output_bar(a_out.cpu(), b_out.cpu(), bar, "written loops")
    for x, y in zip(a_grads, b_grads):
        gr.assert_grad_bar(x.cpu(), y.cpu(), "written loops")
    # nodes 48 (nothing but its written loop) and 49 (no edge at all): xl_i bit for bit, and g_xl[i] = g_out[i]
    for out, grads in ((a_out, a_grads), (b_out, b_grads)):
        assert torch.equal(out[48:], ins[0][48:])
        gr.assert_grad_bar(grads[0][48:].cpu(), g[48:].cpu(), "isolated g_xl")
    # without the flag the written loops count, and the empty row is exactly zero
    out, _alpha, grads, _g = _check(mode, ins, with_loops, what="written loops, no flag")
    assert bool((out[49] == 0).all()) and bool((grads[0][49] == 0).all())
    assert not torch.equal(out[:48], a_out[:48])


# ---- 7. one graph, three forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_same_graph_three_forms(dev, mode, self_loops):
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import edge_list_from_edge_index, lookup_graph
    batch, N = _ragged([40, 33, 70], dev)
    x = ar.coords(N, 60).to(dev)
    ins = [t.to(dev) for t in gr.inputs(mode, N, N, 2, 16, seed=60)]
    table = dm.knn_table(x, 20, batch, loop=True)
    ei = dm.knn_graph(x, 20, batch, loop=True)
    hit = lookup_graph(ei)
    assert hit is not None and torch.equal(hit[0].nbr, table.nbr)
    clone = ei.clone()
    assert lookup_graph(clone) is None
    edges = edge_list_from_edge_index(clone, N, "source_to_target")
    base = _run(mode, ins, table, self_loops=self_loops, want_alpha=False)
    for graph in (table, hit[0], edges):       # the table again: two runs of one form
        other = _run(mode, ins, graph, self_loops=self_loops, want_alpha=False)
        assert torch.equal(base[0], other[0])
        for a, b in zip(base[2], other[2]):
            assert torch.equal(a, b)
    # through the modules: the table, the tensor (found again) and its clone (grouped)
    torch.manual_seed(61)
    conv = (dm.GATv2Conv if mode == gr.V2 else dm.GATConv)(6, 16, heads=2, add_self_loops=self_loops).to(dev)
    xin = torch.randn(N, 6, generator=torch.Generator().manual_seed(62)).to(dev)
    outs = []
    for graph in (table, ei, clone, table):
        conv.zero_grad(set_to_none=True)
        out = conv(xin, graph)
        out.sum().backward()
        outs.append([out.detach()] + [p.grad.clone() for p in conv.parameters()])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


# ---- 8. poisoned allocations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_allocations_change_nothing(dev, mode, self_loops):
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import edge_list_from_edge_index
    batch, N = _ragged([1, 3, 0, 17, 40], dev)
    table = dm.knn_table(ar.coords(N, 64).to(dev), 16, batch, loop=True)
    assert bool((table.nbr < 0).any())
    ei, M = gr.degree_edge_index()
    edges = edge_list_from_edge_index(ei.to(dev), M, "source_to_target")
    assert int((edges.rowptr[1:] == edges.rowptr[:-1]).sum()) >= 1        # an empty row
    for graph, n in ((table, N), (edges, M)):
        ins = [t.to(dev) for t in gr.inputs(mode, n, n, 2, 20, seed=65)]

        def call():
            out, alpha, grads, _g = _run(mode, ins, graph, self_loops=self_loops)
            return [out, alpha] + grads

        clean = [t.cpu() for t in call()]
        for pattern, got in pa.run_both(call).items():
            for a, b in zip(clean, got):
                assert pa.differing(a, b).numel() == 0, (pattern, mode)


# ---- 9. the modules ---------------------------------------------------------------------------------------------------------------------------
def _conv_of(name, dev, seed=70):
    import deepmetv2_amd as dm
    cls, in_channels, opts = gr.MODULE_CASES[name]
    torch.manual_seed(seed)
    conv = (dm.GATv2Conv if cls == "v2" else dm.GATConv)(in_channels, 6, heads=3, **opts)
    with torch.no_grad():
        if conv.bias is not None:
            conv.bias.uniform_(-0.5, 0.5)
    return conv.to(dev)


def _ref_of(conv, name):
    ref = gr.ref_module(name)
    ref.load_state_dict({n: v.detach().cpu().double() for n, v in conv.state_dict().items()}, strict=True)
    return ref


def _module_check(conv, name, x, graph, tgt, src, want_alpha, what=""):
    """Forward, input and parameter gradients (and alpha) of a layer against the float64 reference over (tgt, src)."""
    conv.zero_grad(set_to_none=True)
    pair = isinstance(x, tuple)
    xs = tuple(t.detach().clone().requires_grad_(True) for t in (x if pair else (x,)))
    res = conv(xs if pair else xs[0], graph, return_attention_weights=True if want_alpha else None)
    out, alpha = (res[0], res[1][1]) if want_alpha else (res, None)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(6)).to(out.device)
    out.backward(g)
    ref = _ref_of(conv, name)
    x64 = tuple(t.detach().cpu().double().requires_grad_(True) for t in xs)
    r_out, r_alpha = ref(x64 if pair else x64[0], tgt, src, add_self_loops=conv.add_self_loops, return_alpha=True)
    r_out.backward(g.cpu().double())
    rp = dict(ref.named_parameters())
    got = [("out", out.detach(), r_out.detach())] + [(f"gx{n}", a.grad, b.grad) for n, (a, b) in enumerate(zip(xs, x64))]
    got += [(n, p.grad, rp[n].grad) for n, p in conv.named_parameters()]
    assert len(got) == 1 + len(xs) + len(rp)
    for n, a, b in got:
        gr.assert_grad_bar(a.cpu(), b, f"{what}: {n}")
    return out.detach(), alpha, r_alpha.detach()


@pytest.mark.parametrize("name", list(gr.MODULE_CASES))
def test_module_matches_the_reference(dev, name):
    import deepmetv2_amd as dm
    conv = _conv_of(name, dev)
    _cls, in_channels, opts = gr.MODULE_CASES[name]
    loops = opts["add_self_loops"]
    x, ei, ns, nd = gr.module_inputs(name)
    pair = isinstance(x, tuple)
    xg = tuple(t.to(dev) for t in x) if pair else x.to(dev)
    # a shuffled [2, E] tensor; alpha comes back in the caller's (ungrouped) edge order
    out, alpha, r_alpha = _module_check(conv, name, xg, ei.to(dev), ei[1], ei[0], not loops, what=name)
    assert out.shape == (nd, 18 if opts.get("concat", True) else 6)
    if not loops:
        assert alpha.shape == (ei.shape[1], 3) and not alpha.requires_grad
        torch.testing.assert_close(alpha.cpu().double(), r_alpha, rtol=1e-4, atol=1e-6)
    if pair:        # two sets over a BipartiteTable
        table = dm.knn_xy_table(ar.coords(ns, 72).to(dev), ar.coords(nd, 73).to(dev), 8)
        tgt, src, pos, _ns = _entries(table)
        out, alpha, r_alpha = _module_check(conv, name, xg, table, tgt, src, True, what=name + ", xy table")
        assert alpha.shape == (nd, 8, 3)
        torch.testing.assert_close(alpha.cpu().double(), gr.table_alpha(r_alpha, pos, nd, 8), rtol=1e-4, atol=1e-6)
        with pytest.raises(ValueError, match="source ids"):
            conv((xg[0][:20], xg[1]), ei.to(dev))
        return
    # one set over a table (its written self entries are replaced by the implicit ones when add_self_loops)
    batch, _n = _ragged([30, 27], dev)
    table = dm.knn_table(ar.coords(nd, 72).to(dev), 8, batch, loop=True)
    tgt, src, pos, _ns = _entries(table)
    out, alpha, r_alpha = _module_check(conv, name, xg, table, tgt, src, not loops, what=name + ", table")
    if not loops:
        assert alpha.shape == (nd, 8, 3)
        torch.testing.assert_close(alpha.cpu().double(), gr.table_alpha(r_alpha, pos, nd, 8), rtol=1e-4, atol=1e-6)
        ei2 = table.edge_index()
        _o, (ret, alpha2) = conv(xg, ei2, return_attention_weights=True)
        assert ret is ei2 and alpha2.shape == (ei2.shape[1], 3)
        torch.testing.assert_close(alpha2.cpu().double(), r_alpha, rtol=1e-4, atol=1e-6)
    else:
        with pytest.raises(ValueError, match="add_self_loops=False"):
            conv(xg, table, return_attention_weights=True)


# ---- 10. bf16 autocast ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_bf16_autocast(dev, mode):
    import deepmetv2_amd as dm
    torch.manual_seed(77)
    conv = (dm.GATv2Conv if mode == gr.V2 else dm.GATConv)(12, 16, heads=4).to(dev)
    batch, N = _ragged([60, 33], dev)
    x = torch.randn(N, 12, generator=torch.Generator().manual_seed(78)).to(dev)
    table = dm.knn_table(ar.coords(N, 77).to(dev), 16, batch, loop=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        if mode == gr.V2:
            ins = [conv.lin_l(x).view(-1, 4, 16), conv.lin_r(x).view(-1, 4, 16), conv.att]
        else:
            xl = conv.lin(x).view(-1, 4, 16)
            ins = [xl, (xl * conv.att_src).sum(-1), (xl * conv.att_dst).sum(-1)]
        assert ins[0].dtype == torch.bfloat16
        agg = _op(mode)(*ins, table, self_loops=True)
        out = conv(x, table)
    assert agg.dtype == torch.bfloat16 and out.shape == (N, 64) and bool(torch.isfinite(out.float()).all())
    full = _op(mode)(*[t.float() for t in ins], table, self_loops=True)
    assert full.dtype == torch.float32 and torch.equal(agg, full.to(torch.bfloat16))
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    _op(mode)(*leaves, table, self_loops=True).float().sum().backward()
    for t, src in zip(leaves, ins):
        assert t.grad.dtype == src.dtype and t.grad.shape == src.shape and bool(torch.isfinite(t.grad.float()).all())
    with pytest.raises(TypeError):
        _op(mode)(ins[0].half(), *[t.float() for t in ins[1:]], table)     # fp16 outside fp16 autocast stays an error


# ---- 11. no host sync ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_no_host_sync_with_a_table_and_a_registered_batch(dev, mode):
    import deepmetv2_amd as dm
    sizes = [300, 40, 260]
    torch.manual_seed(76)
    conv = (dm.GATv2Conv if mode == gr.V2 else dm.GATConv)(12, 16, heads=4).to(dev)
    batch, N = _ragged(sizes, dev)
    x = torch.randn(N, 12, generator=torch.Generator().manual_seed(79)).to(dev)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    dm.register_batch(batch, ptr, 3, max_nodes=300, min_nodes=40)
    pos = ar.coords(N, 76).to(dev)
    xx = x.clone().requires_grad_(True)
    conv(xx, dm.knn_table(pos, 16, batch, loop=True)).sum().backward()       # module loads, allocator warm-up
    torch.cuda.synchronize()
    g = torch.randn(N, 64, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = conv(xx, dm.knn_table(pos, 16, batch, loop=True))
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(xx.grad).all())

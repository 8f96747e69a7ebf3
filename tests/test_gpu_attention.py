"""Attention on the GPU (csrc/attention.hip, deepmetv2_amd/attention.py) against the float64 reference of
tests/attention_reference.py over the same graph.

Bars, tests/test_gpu_gravnet.py's.  Output, per row: |err| <= 1e-5 * bar_i + 1e-6 with bar_i = the largest |v_j|_inf of
the row (the output is a convex combination of the row's v_j).  Gradients: rtol 1e-4, atol 1e-4 * max|ref|.  The module's
output passes further fp32 Linears and is held to the gradient bar.  tests/test_attention_host.py shows a float32 run of
the reference inside half of each bar on these inputs.  One gradient needs its scale spelt out: where every key a row
attends to is the same vector (equal scores; the exact-score case, where only ties at the maximum carry weight),
g_q = k sum_e g_s_e / sqrt(C) is a sum that cancels exactly and max|ref| is rounding noise; it is held to 1e-4 of the size
of that sum's terms (attention_reference.g_q_term_scale), as tests/test_gpu_gravnet.py does for lin_s.bias.  The module has
one parameter of that kind: lin_key.bias shifts every score of a row alike and a softmax sees differences only, so its
exact gradient is 0 -- the column sums of g_k cancel -- and it is held to 1e-4 * max|ref g_k|, the bar g_k itself is held to.
"""
import pytest
import torch

import attention_reference as ar

pytestmark = pytest.mark.gpu


def _ragged(sizes, dev):
    counts = torch.tensor(sizes, dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return batch.to(dev), int(counts.sum())


def _entries(graph):
    """(tgt, src, pos or None, Ns) on the CPU of a table or an EdgeList."""
    from deepmetv2_amd.graph import EdgeList
    if isinstance(graph, EdgeList):
        return graph.tgt.cpu().long(), graph.src.cpu().long(), None, graph.num_src
    ns = graph.num_candidates if hasattr(graph, "num_candidates") else graph.num_nodes
    return ar.table_entries(graph.nbr.cpu(), ns) + (ns,)


def _run(q, k, v, graph, g=None, want_alpha=True):
    """GPU forward + backward of the aggregate: (out, alpha, g_q, g_k, g_v, g)."""
    import deepmetv2_amd as dm
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    res = dm.attention_aggregate(qq, kk, vv, graph, return_alpha=want_alpha)
    out, alpha = res if want_alpha else (res, None)
    if g is None:
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    return out.detach(), alpha, qq.grad, kk.grad, vv.grad, g


def _check(q, k, v, graph, what="", cancelling_g_q=False):
    """Output, alpha and the three gradients of attention_aggregate against the float64 reference over `graph`."""
    out, alpha, g_q, g_k, g_v, g = _run(q, k, v, graph)
    tgt, src, pos, _ns = _entries(graph)
    q64, k64, v64 = (t.detach().cpu().double().requires_grad_(True) for t in (q, k, v))
    r_out, r_alpha, bar = ar.attention(q64, k64, v64, tgt, src)
    got = out.cpu()
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), what
    ar.assert_output_bar(got, r_out.detach(), bar, what)
    deg = torch.bincount(tgt, minlength=q.shape[0])
    assert bool((got[deg == 0] == 0).all()), what
    # alpha: the reference's, rows sum to 1 within 1e-6 deg or are all 0, and nothing flows back through it
    assert not alpha.requires_grad
    a = alpha.cpu().double()
    if pos is not None:
        r_full = ar.table_alpha(r_alpha.detach(), pos, q.shape[0], graph.k)
        assert a.shape == r_full.shape, what
        torch.testing.assert_close(a, r_full, rtol=1e-4, atol=1e-6, msg=lambda m: f"{what}: alpha: {m}")
        sums = a.sum(1)
    else:
        torch.testing.assert_close(a, r_alpha.detach(), rtol=1e-4, atol=1e-6, msg=lambda m: f"{what}: alpha: {m}")
        sums = torch.zeros((q.shape[0], a.shape[1]), dtype=torch.float64).index_add(0, tgt, a)
    want = (deg > 0).double().view(-1, 1).expand_as(sums)
    assert bool(((sums - want).abs() <= 1e-6 * deg.clamp(min=1).view(-1, 1)).all()), (what, "alpha rows")
    r_out.backward(g.cpu().double())
    for name, x, ref in (("g_q", g_q, q64.grad), ("g_k", g_k, k64.grad), ("g_v", g_v, v64.grad)):
        scale = ar.g_q_term_scale(q.cpu(), k.cpu(), v.cpu(), tgt, src, g.cpu()) if cancelling_g_q and name == "g_q" else None
        ar.assert_grad_bar(x.cpu(), ref, f"{what}: {name}", scale=scale)
    return out, alpha, g_q, g_k, g_v


# ---- 1. the aggregate over kNN tables ---------------------------------------------------------------------------------------------
# the kernels give a (row, head) pair to 16 lanes (C <= 32; 16 pairs per 256-thread workgroup) or to 32 lanes (C > 32; 8
# pairs per workgroup) and take a row in chunks of that many entries, 4 gathers at a time: k = 1, 8, 16, 20, 33, 64 and
# the in-degrees below sit on both sides of 4, 16, 32 and their multiples, N*H on both sides of 8 and 16 pairs
@pytest.mark.parametrize("case", list(ar.KNN_CASES))
def test_aggregate_on_knn_tables(dev, case):
    import deepmetv2_amd as dm
    sizes, H, C, k = ar.KNN_CASES[case]
    batch, N = _ragged(sizes, dev)
    q, kk, v = (t.to(dev) for t in ar.qkv(N, N, H, C, seed=len(case)))
    table = dm.knn_table(ar.coords(N, len(case)).to(dev), k, batch, loop=True)
    _check(q, kk, v, table, what=case)
    if case == "limits":
        assert bool((table.nbr >= 0).all())
    if case.startswith("short rows"):
        assert bool((table.nbr[:4, 1:] < 0).any()) and bool((table.nbr[:, 0] >= 0).all())


@pytest.mark.parametrize("C", list(ar.CHANNEL_WIDTHS))
def test_every_channel_width(dev, C):
    import deepmetv2_amd as dm
    batch, N = _ragged([40, 9], dev)
    q, k, v = (t.to(dev) for t in ar.qkv(N, N, 2, C, seed=C))
    table = dm.knn_table(ar.coords(N, C).to(dev), 8, batch, loop=True)
    _check(q, k, v, table, what=f"C={C}")


# ---- 3. - 5. edge lists: row lengths across the chunk boundaries, a long row, a long reverse list ---------------------------------
@pytest.fixture(scope="module")
def degree_graph(dev):
    from deepmetv2_amd.graph import edge_list_from_edge_index
    ei, N = ar.degree_edge_index()
    edges = edge_list_from_edge_index(ei.to(dev), N, "source_to_target")
    deg = (edges.rowptr[1:] - edges.rowptr[:-1]).cpu()
    assert deg[:len(ar.IN_DEGREES)].tolist() == list(ar.IN_DEGREES) and edges.perm is not None
    srcptr, _perm = edges.by_source()
    assert int(srcptr[1] - srcptr[0]) == 600
    return edges, N


@pytest.mark.parametrize("H, C", [(2, 16), (1, 40)])
def test_row_lengths_across_chunk_boundaries(dev, degree_graph, H, C):
    edges, N = degree_graph
    q, k, v = (t.to(dev) for t in ar.qkv(N, N, H, C, seed=31))
    _check(q, k, v, edges, what=f"in-degrees, C={C}")


def test_overflow_guard_with_exact_scores(dev, degree_graph):
    edges, N = degree_graph
    q, k, v = (t.to(dev) for t in ar.exact_score_inputs(N))
    out, alpha, g_q, g_k, g_v = _check(q, k, v, edges, what="exact scores", cancelling_g_q=True)
    for t in (out, alpha, g_q, g_k, g_v):
        assert bool(torch.isfinite(t).all())
    assert float(torch.exp(torch.tensor(96.0))) == float("inf")        # what the max subtraction guards against


def test_equal_scores_give_the_row_mean(dev, degree_graph):
    edges, N = degree_graph
    q, k, v = ar.qkv(N, N, 2, 16, seed=33)
    k = k[:1].expand(N, -1, -1).contiguous()
    out, alpha, g_q, _gk, _gv = _check(q.to(dev), k.to(dev), v.to(dev), edges, what="equal scores", cancelling_g_q=True)
    tgt, src = edges.tgt.cpu().long(), edges.src.cpu().long()
    deg = torch.bincount(tgt, minlength=N).double()
    mean = torch.zeros(N, 2, 16, dtype=torch.float64).index_add(0, tgt, v.double()[src]) / deg.clamp(min=1).view(-1, 1, 1)
    bar = torch.zeros(N, dtype=torch.float64).scatter_reduce(0, tgt, v.abs().amax((1, 2)).double()[src], "amax")
    ar.assert_output_bar(out.cpu(), mean, bar, "row mean")
    torch.testing.assert_close(alpha.cpu().double(), (1.0 / deg[tgt]).view(-1, 1).expand(-1, 2), rtol=1e-6, atol=0)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    atol = 1e-4 * ar.g_q_term_scale(q, k, v, tgt, src, g)
    assert float(g_q.abs().max()) <= atol, (float(g_q.abs().max()), atol)


def test_non_finite_values_stay_local(dev):
    import deepmetv2_amd as dm
    batch, N = _ragged([30, 41], dev)
    q, k, v = (t.to(dev) for t in ar.qkv(N, N, 2, 16, seed=34))
    table = dm.knn_table(ar.coords(N, 34).to(dev), 8, batch, loop=True)
    clean = dm.attention_aggregate(q, k, v, table)
    bad = 37
    v2 = v.clone()
    v2[bad, 1, 3] = float("nan")
    got = dm.attention_aggregate(q, k, v2, table)
    holds = (table.nbr == bad).any(1)
    assert 0 < int(holds.sum()) < N
    assert bool(torch.isnan(got[holds][:, 1, 3]).all())
    assert torch.equal(got[~holds], clean[~holds]) and torch.equal(got[:, 0], clean[:, 0])
    assert int(torch.isnan(got).sum()) == int(holds.sum())


# ---- 7. two sets --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, ny", [(40, 9), (9, 40), (1, 5)])
def test_two_sets(dev, nx, ny):
    import deepmetv2_amd as dm
    q, k, v = (t.to(dev) for t in ar.qkv(ny, nx, 3, 22, seed=nx))
    table = dm.knn_xy_table(ar.coords(nx, 50).to(dev), ar.coords(ny, 51).to(dev), 8)
    out, *_ = _check(q, k, v, table, what=f"xy {nx} {ny}")
    assert out.shape == (ny, 3, 22)


def test_two_sets_through_the_module(dev):
    import deepmetv2_amd as dm
    ns, nd = 23, 35
    g = torch.Generator().manual_seed(52)
    ei = torch.stack([torch.randint(0, ns, (300,), generator=g), torch.randint(0, nd - 2, (300,), generator=g)])
    torch.manual_seed(53)
    conv = dm.TransformerConv((7, 9), 5, heads=3).to(dev)
    x_src, x_dst = torch.randn(ns, 7, generator=g), torch.randn(nd, 9, generator=g)
    _module_check(conv, (x_src.to(dev), x_dst.to(dev)), ei.to(dev), ei[1], ei[0], what="pair")
    with pytest.raises(ValueError, match="source ids"):
        conv((x_src[:20].to(dev), x_dst.to(dev)), ei.to(dev))


# ---- 8. one graph, three forms -----------------------------------------------------------------------------------------------------------
def test_same_graph_three_forms(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import edge_list_from_edge_index, lookup_graph
    sizes = [40, 33, 70]
    batch, N = _ragged(sizes, dev)
    x = ar.coords(N, 60).to(dev)
    H, C = 2, 16
    q, k, v = (t.to(dev) for t in ar.qkv(N, N, H, C, seed=60))
    table = dm.knn_table(x, 20, batch, loop=True)
    ei = dm.knn_graph(x, 20, batch, loop=True)
    hit = lookup_graph(ei)
    assert hit is not None and torch.equal(hit[0].nbr, table.nbr)
    clone = ei.clone()
    assert lookup_graph(clone) is None
    edges = edge_list_from_edge_index(clone, N, "source_to_target")
    base = _run(q, k, v, table, want_alpha=False)
    for graph in (hit[0], edges):
        other = _run(q, k, v, graph, want_alpha=False)
        for a, b in zip(base[0:1] + base[2:5], other[0:1] + other[2:5]):
            assert torch.equal(a, b)
    # through the module: the tensor (found again), its clone (grouped), and the table
    torch.manual_seed(61)
    conv = dm.TransformerConv(6, C, heads=H).to(dev)
    xin = torch.randn(N, 6, generator=torch.Generator().manual_seed(62)).to(dev)
    outs = []
    for graph in (table, ei, clone):
        conv.zero_grad(set_to_none=True)
        out = conv(xin, graph)
        out.sum().backward()
        outs.append([out.detach()] + [p.grad.clone() for p in conv.parameters()])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    # the same edges in shuffled order: another summation order, inside the bars
    order = torch.randperm(clone.shape[1], generator=torch.Generator().manual_seed(63)).to(dev)
    shuffled = edge_list_from_edge_index(clone[:, order].contiguous(), N, "source_to_target")
    assert shuffled.perm is not None
    _check(q, k, v, shuffled, what="shuffled")


# ---- 9. - 13. the module -------------------------------------------------------------------------------------------------------------------
def _ref_of(conv):
    ref = ar.RefTransformerConv(conv.in_channels, conv.out_channels, heads=conv.heads, concat=conv.concat,
                                beta=conv.lin_beta is not None, root_weight=conv.lin_skip is not None,
                                bias=conv.lin_skip is not None and conv.lin_skip.bias is not None)
    ref.load_state_dict({n: v.detach().cpu().double() for n, v in conv.state_dict().items()})
    return ref


def _module_check(conv, x, graph, tgt, src, what=""):
    """Forward, alpha, input and parameter gradients of TransformerConv against the float64 reference over (tgt, src)."""
    conv.zero_grad(set_to_none=True)
    pair = isinstance(x, tuple)
    xs = tuple(t.detach().clone().requires_grad_(True) for t in (x if pair else (x,)))
    out, (_g, alpha) = conv(xs if pair else xs[0], graph, return_attention_weights=True)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(6)).to(out.device)
    out.backward(g)
    ref = _ref_of(conv)
    x64 = tuple(t.detach().cpu().double().requires_grad_(True) for t in xs)
    r_out, r_alpha = ref(x64 if pair else x64[0], tgt, src, return_alpha=True)
    r_out.backward(g.cpu().double())
    rp = dict(ref.named_parameters())
    got = [("out", out.detach(), r_out.detach())] + [(f"gx{n}", a.grad, b.grad) for n, (a, b) in enumerate(zip(xs, x64))]
    got += [(n, p.grad, rp[n].grad) for n, p in conv.named_parameters()]
    for name, a, b in got:
        # lin_key.bias: an exactly cancelling sum of g_k rows, held to the scale of its terms (see the docstring)
        scale = float(ref.key.grad.abs().max()) if name == "lin_key.bias" else None
        ar.assert_grad_bar(a.cpu(), b, f"{what}: {name}", scale=scale)
    return out.detach(), alpha, r_alpha.detach()


MODULE_OPTIONS = {
    "concat": dict(concat=True, beta=False, root_weight=True),
    "mean": dict(concat=False, beta=False, root_weight=True),
    "beta": dict(concat=True, beta=True, root_weight=True),
    "no root, no bias": dict(concat=False, beta=True, root_weight=False, bias=False),
}


@pytest.mark.parametrize("name", list(MODULE_OPTIONS))
def test_module_matches_the_reference(dev, name):
    import deepmetv2_amd as dm
    torch.manual_seed(70)
    conv = dm.TransformerConv(10, 6, heads=3, **MODULE_OPTIONS[name]).to(dev)
    g = torch.Generator().manual_seed(71)
    N, E = 57, 400
    x = torch.randn(N, 10, generator=g)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N - 3, (E,), generator=g)])
    # alpha comes back in the caller's (ungrouped) edge order
    out, alpha, r_alpha = _module_check(conv, x.to(dev), ei.to(dev), ei[1], ei[0], what=name)
    assert out.shape == (N, 18 if MODULE_OPTIONS[name]["concat"] else 6) and alpha.shape == (E, 3)
    assert not alpha.requires_grad
    torch.testing.assert_close(alpha.cpu().double(), r_alpha, rtol=1e-4, atol=1e-6)
    # a table: (table, alpha[Nt, k, H]); knn_graph's tensor: alpha[E, H] in that tensor's order
    batch, _n = _ragged([30, 27], dev)
    table = dm.knn_table(ar.coords(N, 72).to(dev), 8, batch, loop=True)
    tgt, src, pos, _ns = _entries(table)
    out, alpha, r_alpha = _module_check(conv, x.to(dev), table, tgt, src, what=name + ", table")
    assert alpha.shape == (N, 8, 3)
    torch.testing.assert_close(alpha.cpu().double(), ar.table_alpha(r_alpha, pos, N, 8), rtol=1e-4, atol=1e-6)
    ei2 = table.edge_index()
    _o, (ret, alpha2) = conv(x.to(dev), ei2, return_attention_weights=True)
    assert ret is ei2 and alpha2.shape == (ei2.shape[1], 3)
    r2 = ar.attention(*(_ref_qkv(conv, x)), ei2[1].cpu(), ei2[0].cpu())[1]
    torch.testing.assert_close(alpha2.cpu().double(), r2, rtol=1e-4, atol=1e-6)


def _ref_qkv(conv, x):
    ref = _ref_of(conv)
    H, C = conv.heads, conv.out_channels
    with torch.no_grad():
        x = x.double()
        return ref.lin_query(x).view(-1, H, C), ref.lin_key(x).view(-1, H, C), ref.lin_value(x).view(-1, H, C)


def test_module_loads_a_reference_state_dict(dev):
    import deepmetv2_amd as dm
    torch.manual_seed(73)
    ref = ar.RefTransformerConv(12, 8, heads=4, beta=True)
    conv = dm.TransformerConv(12, 8, heads=4, beta=True)
    conv.load_state_dict({n: v.float() for n, v in ref.state_dict().items()}, strict=True)
    conv = conv.to(dev)
    batch, N = _ragged([50, 23], dev)
    x = torch.randn(N, 12, generator=torch.Generator().manual_seed(74))
    table = dm.knn_table(ar.coords(N, 74).to(dev), 16, batch, loop=True)
    out = conv(x.to(dev), table)
    tgt, src, _pos, _ns = _entries(table)
    r_out = _ref_of(conv)(x.double(), tgt, src).detach()      # over the parameters as rounded to fp32
    ar.assert_grad_bar(out.detach().cpu(), r_out, "loaded")
    ar.assert_grad_bar(ref(x.double(), tgt, src).detach(), r_out, "rounding the parameters")


def _module_inputs(dev, sizes, seed):
    import deepmetv2_amd as dm
    torch.manual_seed(seed)
    conv = dm.TransformerConv(12, 16, heads=4, beta=True).to(dev)
    batch, N = _ragged(list(sizes), dev)
    x = torch.randn(N, 12, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    return conv, x, batch


def test_two_runs_give_identical_bits(dev):
    import deepmetv2_amd as dm
    conv, x, batch = _module_inputs(dev, (300, 40, 129), seed=75)
    table = dm.knn_table(ar.coords(x.shape[0], 75).to(dev), 16, batch, loop=True)
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        out = conv(xx, table)
        out.backward(torch.ones_like(out) * 0.37)
        runs.append([out.detach(), xx.grad] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_host_sync_with_a_table_and_a_registered_batch(dev):
    import deepmetv2_amd as dm
    sizes = [300, 40, 260]
    conv, x, batch = _module_inputs(dev, sizes, seed=76)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    dm.register_batch(batch, ptr, 3, max_nodes=300, min_nodes=40)
    pos = ar.coords(x.shape[0], 76).to(dev)
    xx = x.clone().requires_grad_(True)
    conv(xx, dm.knn_table(pos, 16, batch, loop=True)).sum().backward()       # module loads, allocator warm-up
    torch.cuda.synchronize()
    g = torch.randn(sum(sizes), 64, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = conv(xx, dm.knn_table(pos, 16, batch, loop=True))
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(xx.grad).all())


def test_bf16_autocast(dev):
    import deepmetv2_amd as dm
    conv, x, batch = _module_inputs(dev, (60, 33), seed=77)
    table = dm.knn_table(ar.coords(x.shape[0], 77).to(dev), 16, batch, loop=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        q, k, v = (lin(x).view(-1, 4, 16) for lin in (conv.lin_query, conv.lin_key, conv.lin_value))
        assert q.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
        agg = dm.attention_aggregate(q, k, v, table)
        out = conv(x, table)
    assert agg.dtype == torch.bfloat16 and out.shape == (x.shape[0], 64)
    full = dm.attention_aggregate(q.float(), k.float(), v.float(), table)
    assert full.dtype == torch.float32 and torch.equal(agg, full.to(torch.bfloat16))
    mixed = dm.attention_aggregate(q, k, v.float(), table)                 # the result follows v
    assert mixed.dtype == torch.float32 and torch.equal(mixed, full)
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    dm.attention_aggregate(qq, kk, vv, table).float().sum().backward()
    for t in (qq, kk, vv):
        assert t.grad.dtype == torch.bfloat16 and bool(torch.isfinite(t.grad.float()).all())
    with pytest.raises(TypeError):
        dm.attention_aggregate(q.half(), k.float(), v.float(), table)     # fp16 outside fp16 autocast stays an error


# ---- 14. memory -----------------------------------------------------------------------------------------------------------------------------
def _composed(q, k, v, nbr):
    """The route without the kernels, over a table without empty slots: three index_selects, scatter amax, two index_adds."""
    N, kk = nbr.shape
    H, C = q.shape[1], q.shape[2]
    src = nbr.reshape(-1).long()
    tgt = torch.arange(N, device=q.device).repeat_interleave(kk)
    score = (q.index_select(0, tgt) * k.index_select(0, src)).sum(-1) / (C ** 0.5)
    m = torch.full((N, H), float("-inf"), device=q.device).scatter_reduce(0, tgt.view(-1, 1).expand(-1, H), score.detach(), "amax")
    p = torch.exp(score - m.index_select(0, tgt))
    l = torch.zeros((N, H), device=q.device).index_add_(0, tgt, p)
    alpha = p / l.index_select(0, tgt)
    return torch.zeros_like(q).index_add_(0, tgt, alpha.unsqueeze(-1) * v.index_select(0, src))


def test_memory_stays_below_one_message_tensor(dev):
    """8 x 2000 nodes, k 16, H 4, C 16: forward + backward of the aggregate grows the peak by less than one [E, H*C] fp32
    tensor; the composed route (which also agrees with it) by more."""
    import deepmetv2_amd as dm
    batch, N = _ragged([2000] * 8, dev)
    q, k, v = (t.to(dev) for t in ar.qkv(N, N, 4, 16, seed=78))
    table = dm.knn_table(ar.coords(N, 78).to(dev), 16, batch, loop=True)
    table.reverse()
    nbr = table.nbr
    assert bool((nbr >= 0).all())
    one = N * 16 * 64 * 4
    g = torch.randn(N, 4, 16, device=dev)
    grown, outs = {}, {}
    for name, fn in (("fused", lambda a, b, c: dm.attention_aggregate(a, b, c, table)),
                     ("composed", lambda a, b, c: _composed(a, b, c, nbr))):
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.max_memory_allocated(dev)
        out = fn(qq, kk, vv)
        out.backward(g)
        torch.cuda.synchronize(dev)
        grown[name] = torch.cuda.max_memory_allocated(dev) - base
        outs[name] = (out.detach(), qq.grad, kk.grad, vv.grad)
        del out
    assert grown["fused"] < one, grown
    assert grown["composed"] > one, grown
    bar = v.abs().amax((1, 2))[nbr.long()].amax(1)
    ar.assert_output_bar(outs["fused"][0].cpu(), outs["composed"][0].cpu(), bar.cpu(), "fused vs composed")
    for a, b in zip(outs["fused"][1:], outs["composed"][1:]):
        ar.assert_grad_bar(a.cpu(), b.cpu(), "fused vs composed")


def test_a_score_of_minus_infinity_follows_the_formula(dev):
    """An empty slot is told by its id, not by its score: an entry whose q . k overflowed to -inf weighs 0 beside a finite
    score, and a row of nothing but such entries is NaN in out, lse and alpha (torch.softmax of all -inf), never 0."""
    from deepmetv2_amd import _native
    q = torch.full((3, 1, 1), 3e38, device=dev)
    k = torch.tensor([-3e38, 0.0], device=dev).view(2, 1, 1)
    v = torch.tensor([5.0, 7.0], device=dev).view(2, 1, 1)
    nbr = torch.tensor([[0, 1, -1], [0, -1, 0], [-1, -1, -1]], dtype=torch.int32, device=dev)
    out, lse, alpha = (t.cpu() for t in _native.attention_fwd(q, k, v, nbr, None, True))
    assert out[0].item() == 7.0 and lse[0].item() == 0.0 and alpha[0:3, 0].tolist() == [0.0, 1.0, 0.0]
    assert bool(out[1].isnan().all()) and bool(lse[1].isnan().all())
    assert bool(alpha[3].isnan()) and alpha[4].item() == 0.0 and bool(alpha[5].isnan())
    assert out[2].item() == 0.0 and lse[2].item() == 0.0 and alpha[6:9, 0].tolist() == [0.0, 0.0, 0.0]

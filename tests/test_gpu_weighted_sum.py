"""weighted_aggregate, spmm, gcn_norm and GCNConv / GraphConv / SAGEConv / GINConv on the GPU (csrc/weighted_sum.hip,
deepmetv2_amd/propagate.py, deepmetv2_amd/gcn.py) against the float64 restatements of tests/weighted_sum_reference.py on
the graphs of tests/pna_cases.py.

Bounds per element, u = 2^-24, against float64 on the same fp32 inputs:
  out: (n_i + 2) u sum_e |w_e x[j_e,f]|      g_x: (n_j + 2) u sum_p |w_p g_out[i,f]|      g_w[p]: (F + 8) u sum_f |g_out[i,f] x[j,f]|
  empty rows, unlisted sources and empty slots: exactly 0;  count: equal.
tests/test_weighted_sum_host.py holds an fp32 emulation of the kernels' chains under half of each of them on these inputs.
Every element is checked; each check prints its largest error / bound ratio before it asserts.

The layers' tolerance is measured, not derived: per tensor, 4 times the largest error of the same layer composed from fp32
torch operators on the CPU (index_select, multiply, index_add_) against the float64 restatement -- the fused layer is only
another summation order -- plus 1e-6 of the tensor's largest magnitude.
"""
import pytest
import torch

import poisoned_alloc as pa
import weighted_sum_reference as wr

pytestmark = pytest.mark.gpu


def _graph(graph, Nt, Ns, dev, bipartite=False):
    from deepmetv2_amd.graph import BipartiteTable, EdgeList, NeighborTable
    if "nbr" in graph:
        nbr = graph["nbr"].to(dev)
        return BipartiteTable(nbr, None, None, Ns) if bipartite else NeighborTable(nbr, None, dense=False)
    src, rowptr = graph["src"].to(dev), graph["rowptr"].to(dev)
    tgt = torch.repeat_interleave(torch.arange(Nt, dtype=torch.int32, device=dev), rowptr.diff().long())
    return EdgeList(src, tgt, rowptr, Nt, num_src=Ns)


def _run(x, w, graph, g_out):
    """(out, g_x, g_w) of weighted_aggregate and its backward; x and g_out may be unaligned views."""
    import deepmetv2_amd as dm
    xx = x.detach().requires_grad_(True)        # shares x's storage: an unaligned view stays one
    ww = None if w is None else w.detach().requires_grad_(True)
    out = dm.weighted_aggregate(xx, graph, ww)
    out.backward(g_out)
    return out.detach(), xx.grad, None if ww is None else ww.grad


def _ratio(name, what, err, lim):
    r = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: {name} max err/bound {r:.3f}")
    assert bool((err <= lim).all()), (what, name, r)


def _check(case, dev, bipartite=False, what=""):
    from deepmetv2_amd import _native
    x, w, g_out, graph, pos, Nt = case
    Ns, F = x.shape
    gr = _graph(graph, Nt, Ns, dev, bipartite)
    w_in = w.view(Nt, -1) if "nbr" in graph else w
    out, g_x, g_w = _run(x.to(dev), w_in.to(dev), gr, g_out.to(dev))
    assert out.shape == (Nt, F) and g_x.shape == (Ns, F) and g_w.shape == w_in.shape, what
    idx, rowptr = (graph["nbr"], None) if "nbr" in graph else (graph["src"], graph["rowptr"])
    raw, count = _native._weighted_sum_fwd(x.to(dev), w.to(dev), idx.to(dev), None if rowptr is None else rowptr.to(dev), Nt)
    assert torch.equal(raw, out), what
    ref, n, b_out = wr.forward(x, w, *pos, Nt)
    assert count.dtype == torch.int32 and torch.equal(count.cpu().long(), n), what
    want_x, n_j, b_x = wr.grad_x(g_out, w, *pos, Ns)
    want_w, b_w = wr.grad_w(g_out, x, *pos)
    for name, got, want, lim in (("out", out, ref, b_out), ("g_x", g_x, want_x, b_x), ("g_w", g_w.reshape(-1), want_w, b_w)):
        got = got.cpu().double()
        assert bool(torch.isfinite(got).all()), (what, name)
        _ratio(name, what, (got - want).abs(), lim)
    assert bool((out.cpu()[n == 0] == 0).all()) and bool((g_x.cpu()[n_j == 0] == 0).all()), what
    assert bool((g_w.cpu().reshape(-1)[~pos[2]] == 0).all()), what
    return n, n_j


# ---- 1. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", wr.WIDTHS)
def test_table_widths(dev, k):
    n, _n_j = _check(wr.kernel_case("table", 5, k), dev, what=f"table k={k} F=5")
    assert bool((n == 0).any()) and int(n.max()) <= k
    if k in (16, 17):
        _check(wr.kernel_case("table", 64, k), dev, what=f"table k={k} F=64")


@pytest.mark.parametrize("F", wr.FEATURES)
def test_feature_widths(dev, F):
    _check(wr.kernel_case("table", F, 3), dev, what=f"table F={F}")
    n, n_j = _check(wr.kernel_case("list", F, 0), dev, what=f"list F={F}")
    assert {0, 1, 2, 63, 64, 65, 300} <= set(n.tolist()) and bool((n_j == 0).any())


def test_bipartite_table(dev):
    case = wr.kernel_case("table", 12, 16, 57)
    assert case[0].shape[0] == 57 and case[5] == 201
    _check(case, dev, bipartite=True, what="bipartite")


def test_weights_hold_zeros_and_negative_values():
    w = wr.kernel_case("table", 5, 16)[1]
    assert bool((w == 0).any()) and bool((w < 0).any()) and bool((w > 0).any())


# ---- 2. properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,k", [("table", 17), ("list", 0)])
def test_no_weights_give_the_bits_of_ones(dev, kind, k):
    x, w, g_out, graph, _pos, Nt = wr.kernel_case(kind, 64, k)
    gr = _graph(graph, Nt, Nt, dev)
    a = _run(x.to(dev), None, gr, g_out.to(dev))
    b = _run(x.to(dev), torch.ones_like(w).to(dev), gr, g_out.to(dev))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] is None


@pytest.mark.parametrize("kind,k,F", [("table", 17, 64), ("table", 3, 5), ("list", 0, 4)])
def test_nan_in_the_weights_of_empty_slots_changes_nothing(dev, kind, k, F):
    x, w, g_out, graph, (tgt, src, valid), Nt = wr.kernel_case(kind, F, k)
    if kind == "list":      # a list has no blank slots of its own: give it ids that are no entry
        graph = {"src": graph["src"].clone(), "rowptr": graph["rowptr"]}
        graph["src"][::7] = -1
        graph["src"][3::11] = Nt + 5
        valid = wr.positions_of_list(graph["src"], graph["rowptr"], Nt)[2]
    assert bool((~valid).any())
    gr = _graph(graph, Nt, Nt, dev)
    poisoned = torch.where(valid, w, torch.full_like(w, float("nan")))
    a = _run(x.to(dev), w.to(dev), gr, g_out.to(dev))
    b = _run(x.to(dev), poisoned.to(dev), gr, g_out.to(dev))
    for p, q in zip(a, b):
        assert torch.equal(p, q) and bool(torch.isfinite(q).all())
    assert bool((b[2].cpu()[~valid] == 0).all())


@pytest.mark.parametrize("kind,k,F", [("table", 17, 64), ("list", 0, 128), ("table", 3, 256)])
def test_unaligned_views_give_the_same_bits(dev, kind, k, F):
    x, w, g_out, graph, _pos, Nt = wr.kernel_case(kind, F, k)
    gr = _graph(graph, Nt, Nt, dev)

    def shifted(t):
        flat = torch.zeros(t.numel() + 1, device=dev)
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    x, g_out, w = x.to(dev), g_out.to(dev), w.to(dev)
    assert x.data_ptr() % 16 == 0 and g_out.data_ptr() % 16 == 0
    a = _run(x, w, gr, g_out)
    for b in (_run(shifted(x), w, gr, shifted(g_out)), _run(shifted(x), w, gr, g_out), _run(x, w, gr, shifted(g_out))):
        for p, q in zip(a, b):
            assert torch.equal(p, q)


@pytest.mark.parametrize("k,F", [(17, 64), (64, 5), (3, 129)])
def test_a_table_and_its_list_give_the_same_bits(dev, k, F):
    from deepmetv2_amd.graph import EdgeList
    x, w, g_out, graph, (tgt, src, valid), Nt = wr.kernel_case("table", F, k)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(tgt[valid], minlength=Nt).cumsum(0)])
    edges = EdgeList(src[valid].to(torch.int32).to(dev), tgt[valid].to(torch.int32).to(dev), rowptr.to(torch.int32).to(dev), Nt)
    a = _run(x.to(dev), w.to(dev), _graph(graph, Nt, Nt, dev), g_out.to(dev))
    b = _run(x.to(dev), w[valid].to(dev), edges, g_out.to(dev))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][valid.to(dev)], b[2])


def test_two_runs_give_identical_bits(dev):
    x, w, g_out, graph, _pos, Nt = wr.kernel_case("list", 64, 0)
    gr = _graph(graph, Nt, Nt, dev)
    a, b = _run(x.to(dev), w.to(dev), gr, g_out.to(dev)), _run(x.to(dev), w.to(dev), gr, g_out.to(dev))
    for p, q in zip(a, b):
        assert torch.equal(p, q)


def test_no_targets_and_no_edges(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    from deepmetv2_amd.graph import BipartiteTable, EdgeList
    x = torch.randn(5, 4, device=dev)
    none = BipartiteTable(torch.zeros((0, 3), dtype=torch.int32, device=dev), None, None, 5)
    assert dm.weighted_aggregate(x, none, torch.zeros((0, 3), device=dev)).shape == (0, 4)
    g_x, g_w = _native._weighted_sum_bwd(torch.zeros((0, 4), device=dev), x, None, none.nbr, None, None,
                                         torch.zeros(6, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                                         True, False)
    assert g_w is None and g_x.shape == (5, 4) and bool((g_x == 0).all())
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    edges = EdgeList(e, e, torch.zeros(8, dtype=torch.int32, device=dev), 7, num_src=5)
    out, g_x, g_w = _run(x, torch.zeros(0, device=dev), edges, torch.randn(7, 4, device=dev))
    assert out.shape == (7, 4) and bool((out == 0).all()) and bool((g_x == 0).all()) and g_w.shape == (0,)


@pytest.mark.parametrize("kind,k", [("table", 17), ("list", 0)])
def test_bits_do_not_depend_on_what_the_buffers_held(dev, kind, k):
    """Outputs allocated over 0xFF bytes and over 3e38 / zero bytes: the same bits, so every element is written."""
    from deepmetv2_amd import _native
    x, w, g_out, graph, _pos, Nt = wr.kernel_case(kind, 12, k)
    gr = _graph(graph, Nt, Nt, dev)
    x, w, g_out = x.to(dev), w.to(dev), g_out.to(dev)
    table = kind == "table"
    idx, rowptr, tgt = (gr.nbr, None, None) if table else (gr.src, gr.rowptr, gr.tgt)
    rev_ptr, rev_pos = gr.reverse() if table else gr.by_source()

    def call():
        out, count = _native._weighted_sum_fwd(x, w, idx, rowptr, Nt)
        g_x, g_w = _native._weighted_sum_bwd(g_out, x, w, idx, rowptr, tgt, rev_ptr, rev_pos, True, True)
        return out, count, g_x, g_w

    got = pa.run_both(call)
    assert len(got["ones"]) == len(got["zeros_huge"]) == 4
    for a, b in zip(got["ones"], got["zeros_huge"]):
        assert pa.differing(a, b).numel() == 0
        assert not a.is_floating_point() or bool(torch.isfinite(a).all())


def test_only_the_gradients_that_are_needed(dev):
    import deepmetv2_amd as dm
    x, w, g_out, graph, _pos, Nt = wr.kernel_case("table", 64, 16)
    gr = _graph(graph, Nt, Nt, dev)
    x, w, g_out = x.to(dev), w.to(dev), g_out.to(dev)
    _out, g_x, g_w = _run(x, w, gr, g_out)
    xx = x.clone().requires_grad_(True)
    dm.weighted_aggregate(xx, gr, w).backward(g_out)
    assert torch.equal(xx.grad, g_x) and w.grad is None
    ww = w.clone().requires_grad_(True)
    dm.weighted_aggregate(x, gr, ww).backward(g_out)
    assert torch.equal(ww.grad, g_w) and x.grad is None


def test_mean_divides_by_the_entry_count(dev):
    import deepmetv2_amd as dm
    x, w, _g, graph, pos, Nt = wr.kernel_case("table", 5, 16)
    gr = _graph(graph, Nt, Nt, dev)
    ref, n, _b = wr.forward(x, w, *pos, Nt)
    s = dm.weighted_aggregate(x.to(dev), gr, w.to(dev), reduce="add")
    m = dm.weighted_aggregate(x.to(dev), gr, w.to(dev), reduce="mean")
    assert torch.equal(m, s / n.clamp(min=1).to(dev).float().view(-1, 1)) and bool((m.cpu()[n == 0] == 0).all())


def test_no_host_sync(dev):
    from deepmetv2_amd.graph import NeighborTable
    x, w, g_out, graph, _pos, Nt = wr.kernel_case("table", 64, 16)
    x, w, g_out, nbr = x.to(dev), w.to(dev), g_out.to(dev), graph["nbr"].to(dev)
    _run(x, w, NeighborTable(nbr, None, dense=False), g_out)          # module loads, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, g_x, g_w = _run(x, w, NeighborTable(nbr, None, dense=False), g_out)       # a fresh table: its reverse index too
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out).all()) and bool(g_x.abs().sum() > 0) and bool(g_w.abs().sum() > 0)


def test_bf16(dev):
    import deepmetv2_amd as dm
    x, w, _g, graph, _pos, Nt = wr.kernel_case("table", 64, 16)
    gr = _graph(graph, Nt, Nt, dev)
    xb, w = x.to(dev).to(torch.bfloat16), w.to(dev)
    out = dm.weighted_aggregate(xb, gr, w)
    full = dm.weighted_aggregate(xb.float(), gr, w)
    assert out.dtype == torch.bfloat16 and full.dtype == torch.float32 and torch.equal(out, full.to(torch.bfloat16))
    xx, ww = xb.clone().requires_grad_(True), w.clone().requires_grad_(True)
    dm.weighted_aggregate(xx, gr, ww).float().sum().backward()
    assert xx.grad.dtype == torch.bfloat16 and ww.grad.dtype == torch.float32
    assert bool(torch.isfinite(xx.grad.float()).all()) and bool(torch.isfinite(ww.grad).all())
    with pytest.raises(TypeError):
        dm.weighted_aggregate(x.to(dev).half(), gr, w)              # fp16 outside fp16 autocast stays an error


def test_spmm_with_a_shuffled_index(dev):
    """value's gradient comes back in the caller's order; duplicate coordinates add.  Bounds: the forward's and the
    backward's of the module docstring over the grouped list (a stable grouping keeps the caller's order in a row)."""
    import deepmetv2_amd as dm
    x, w, g_out, graph, (tgt, src, valid), Nt = wr.kernel_case("list", 5, 0)
    perm = torch.randperm(tgt.numel(), generator=torch.Generator().manual_seed(5))
    index = torch.stack([tgt[perm], src[perm]])
    value = w[perm]
    v, mat = value.to(dev).requires_grad_(True), x.to(dev).requires_grad_(True)
    out = dm.spmm(index.to(dev), v, Nt, Nt, mat)
    out.backward(g_out.to(dev))
    ref, _n, b_out = wr.forward(x, w, tgt, src, valid, Nt)
    _ratio("out", "spmm", (out.detach().cpu().double() - ref).abs(), b_out)
    want_x, _nj, b_x = wr.grad_x(g_out, w, tgt, src, valid, Nt)
    _ratio("g_matrix", "spmm", (mat.grad.cpu().double() - want_x).abs(), b_x)
    want_w, b_w = wr.grad_w(g_out, x, tgt, src, valid)
    _ratio("g_value", "spmm", (v.grad.cpu().double() - want_w[perm]).abs(), b_w[perm])


# ---- 3. the layers ---------------------------------------------------------------------------------------------------------
def _hold(got, want, cpu32, what):
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_n, b), (_m, c) in zip(got, want, cpu32):
        assert a is not None, (what, name)
        scale = float(b.abs().max())
        err = float((a.cpu().double() - b).abs().max())
        base = float((c.double() - b).abs().max())
        tol = 4 * base + 1e-6 * scale
        print(f"{what} {name}: error {err:.2e}, fp32 torch composition on the CPU {base:.2e}, tolerance {tol:.2e}, "
              f"ratio {err / max(tol, 1e-300):.3f}")
        assert err <= tol, (what, name, err, tol)


def _layer_case(dev, name, kind, seed=9):
    case = wr.layer_graph(kind)
    N, (tgt, src, valid) = case["N"], case["pos"]
    weighted = wr.LAYERS[name][4]
    ours, ref64, ref32 = wr.build_layer(name)
    cin, cout = wr.LAYERS[name][2]
    g = torch.Generator().manual_seed(seed)
    x, gout = torch.randn(N, cin, generator=g), torch.randn(N, cout, generator=g)
    w = case["w"] if weighted else None
    wv = None if w is None else w[valid]
    want = wr.layer_tensors(ref64, x.double(), (src[valid], tgt[valid]), None if wv is None else wv.double(), gout.double())
    cpu32 = wr.layer_tensors(ref32, x, (src[valid], tgt[valid]), wv, gout)
    ours = ours.to(dev)
    gr = _graph(case["graph"], N, N, dev)
    got = wr.layer_tensors(ours, x.to(dev), (gr,), None if w is None else w.to(dev), gout.to(dev), valid)
    _hold(got, want, cpu32, f"{name} {kind}")
    return ours, gr, x, w, gout, got, (tgt, src, valid)


@pytest.mark.parametrize("kind", ["table", "list"])
@pytest.mark.parametrize("name", list(wr.LAYERS))
def test_layers_against_their_float64_restatements(dev, name, kind):
    """Measured on an MI355X, the largest error / tolerance ratio over out, g_x, g_w and every parameter's gradient, table
    and list together: gcn 0.17, gcn_unweighted 0.12, gcn_improved 0.16, gcn_no_self_loops 0.22, gcn_no_normalize 0.13,
    graph_add 0.16, graph_mean 0.21, sage_mean 0.15, sage_sum 0.12, sage_max 0.15, sage_normalize_project 0.13,
    gin 0.16.  The fp32 torch composition's own errors, which set the tolerance, are between 1e-7 and 5e-5
    in absolute terms on these tensors (the printed lines)."""
    ours, _gr, _x, _w, _gout, got, (tgt, _src, valid) = _layer_case(dev, name, kind)
    if name == "gcn_no_self_loops":          # an isolated node: the bias alone
        empty = torch.bincount(tgt[valid], minlength=got[0][1].shape[0]) == 0
        assert bool(empty.any()) and torch.equal(got[0][1].cpu()[empty], ours.bias.detach().cpu().expand(int(empty.sum()), -1))


def test_gcn_cached_twice(dev):
    import deepmetv2_amd as dm
    case = wr.layer_graph("table")
    N = case["N"]
    gr = _graph(case["graph"], N, N, dev)
    torch.manual_seed(12)
    conv, plain = dm.GCNConv(wr.CIN, wr.COUT, cached=True).to(dev), dm.GCNConv(wr.CIN, wr.COUT).to(dev)
    plain.load_state_dict(conv.state_dict())
    x, w = torch.randn(N, wr.CIN, device=dev), case["w"].to(dev)
    a = conv(x, gr, w)
    assert conv._cached_norm is not None
    b = conv(x, gr, w)
    assert torch.equal(a, b) and torch.equal(a, plain(x, gr, w))


@pytest.mark.parametrize("name", ["graph_add", "sage_mean", "gin"])
def test_layers_on_a_pair_over_a_bipartite_table(dev, name):
    x_src, w, _g, graph, (tgt, src, valid), Nt = wr.kernel_case("table", 12, 16, 57)
    gr = _graph(graph, Nt, 57, dev, bipartite=True)
    g = torch.Generator().manual_seed(10)
    ours, ref64, ref32 = wr.build_layer(name, channels=(12, 12) if name == "gin" else (12, 6))
    x_dst, gout = torch.randn(Nt, 12 if name == "gin" else 6, generator=g), torch.randn(Nt, wr.COUT, generator=g)
    ww = w.abs() if wr.LAYERS[name][4] else None
    wv = None if ww is None else ww[valid]
    want = wr.layer_tensors(ref64, (x_src.double(), x_dst.double()), (src[valid], tgt[valid]),
                            None if wv is None else wv.double(), gout.double())
    cpu32 = wr.layer_tensors(ref32, (x_src, x_dst), (src[valid], tgt[valid]), wv, gout)
    got = wr.layer_tensors(ours.to(dev), (x_src.to(dev), x_dst.to(dev)), (gr,), None if ww is None else ww.to(dev), gout.to(dev),
                           valid)
    _hold(got, want, cpu32, f"{name} pair")


@pytest.mark.parametrize("name", ["gcn", "graph_mean"])
def test_a_shuffled_edge_index_equals_the_grouped_run(dev, name):
    """A shuffled [2, E] tensor with edge_weight in its order: the grouped run's results under the same tolerance (the
    order inside a row differs), the weight gradient back in the caller's order."""
    ours, _gr, x, w, gout, _got, (tgt, src, valid) = _layer_case(dev, name, "list")
    case = wr.layer_graph("list")
    ref64, ref32 = wr.build_layer(name)[1:]
    perm = torch.randperm(tgt.numel(), generator=torch.Generator().manual_seed(11))
    ei = torch.stack([src[perm], tgt[perm]])
    want = wr.layer_tensors(ref64, x.double(), (src[perm], tgt[perm]), w[perm].double(), gout.double())
    cpu32 = wr.layer_tensors(ref32, x, (src[perm], tgt[perm]), w[perm], gout)
    got = wr.layer_tensors(ours, x.to(dev), (ei.to(dev),), w[perm].to(dev), gout.to(dev))
    assert case["N"] == x.shape[0] and bool(valid.all())
    _hold(got, want, cpu32, f"{name} shuffled")


def test_knn_graph_tensor_runs_over_its_table(dev):
    """The [2, E] tensor of knn_graph is recognised: without weights it runs over the table; with weights sized N*k, in
    position order, too -- the same bits as the table itself."""
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(13)
    N, k = 300, 8
    pos = torch.randn(N, 2, generator=g).to(dev)
    table = dm.knn_table(pos, k, None, loop=True)
    ei = table.edge_index()
    x, w = torch.randn(N, wr.CIN, generator=g).to(dev), (0.1 + torch.rand(N * k, generator=g)).to(dev)
    torch.manual_seed(14)
    conv = dm.GraphConv(wr.CIN, wr.COUT).to(dev)
    assert ei.shape[1] == N * k
    assert torch.equal(conv(x, ei), conv(x, table)) and torch.equal(conv(x, ei, w), conv(x, table, w.view(N, k)))
    sage = dm.SAGEConv(wr.CIN, wr.COUT, aggr="max").to(dev)
    assert torch.equal(sage(x, ei), sage(x, table))

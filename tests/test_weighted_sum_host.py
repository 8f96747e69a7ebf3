"""weighted_aggregate, spmm, gcn_norm and GCNConv / GraphConv / SAGEConv / GINConv without a GPU: the fp32 emulation of
csrc/weighted_sum.hip's chains under half of every bound of tests/test_gpu_weighted_sum.py on that file's inputs, the
layers over the emulated kernels against their float64 restatements (tests/weighted_sum_reference.py), every refusal,
the C entries' argument checks, and gcn_norm on a hand-made graph."""
import os
import shutil

import numpy as np
import pytest
import torch

import fake_native
import weighted_sum_reference as wr


# ---- 1. the bounds are reachable by the kernels' chains -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,F,k,num_src", wr.KERNEL_CASES)
def test_kernel_chain_emulation_stays_under_half_of_every_bound(kind, F, k, num_src):
    x, w, g_out, _graph, pos, Nt = wr.kernel_case(kind, F, k, num_src)
    Ns = x.shape[0]
    for weights in (w, None):
        wn = None if weights is None else weights.numpy()
        out, count, b_out = wr.forward(x, weights, *pos, Nt)
        got, n = wr.emulate_fwd(x.numpy(), wn, *pos, Nt)
        assert np.array_equal(n, count.numpy())
        g_x, n_j, b_x = wr.grad_x(g_out, weights, *pos, Ns)
        got_x = wr.emulate_bwd_x(g_out.numpy(), wn, *pos, Ns)
        for name, a, ref, lim in (("out", got, out, b_out), ("g_x", got_x, g_x, b_x)):
            err = (torch.from_numpy(a).double() - ref).abs()
            ratio = float((err / lim.clamp(min=1e-300)).max())
            print(f"{kind} F={F} k={k} {name}: emulated error / bound {ratio:.3f}")
            assert ratio <= 0.5 and bool((err[lim == 0] == 0).all()), (name, ratio)
        assert bool((got[count.numpy() == 0] == 0).all()) and bool((got_x[n_j.numpy() == 0] == 0).all())
    g_w, b_w = wr.grad_w(g_out, x, *pos)
    got_w = wr.emulate_bwd_w(g_out.numpy(), x.numpy(), *pos)
    err = (torch.from_numpy(got_w).double() - g_w).abs()
    ratio = float((err / b_w.clamp(min=1e-300)).max())
    print(f"{kind} F={F} k={k} g_w: emulated error / bound {ratio:.3f}")
    assert ratio <= 0.5 and bool((got_w[~pos[2].numpy()] == 0).all())


def test_reference_gradients_equal_autograd():
    x, w, g_out, _graph, (tgt, src, valid), Nt = wr.kernel_case("list", 5, 0)
    p = torch.nonzero(valid).view(-1)
    xx, ww = x.double().requires_grad_(True), w.double().requires_grad_(True)
    out = torch.zeros(Nt, 5, dtype=torch.float64).index_add(0, tgt[p], ww[p].view(-1, 1) * xx[src[p]])
    torch.testing.assert_close(out, wr.forward(x, w, tgt, src, valid, Nt)[0], rtol=1e-12, atol=1e-12)
    out.backward(g_out.double())
    torch.testing.assert_close(xx.grad, wr.grad_x(g_out, w, tgt, src, valid, x.shape[0])[0], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ww.grad, wr.grad_w(g_out, x, tgt, src, valid)[0], rtol=1e-12, atol=1e-12)


# ---- 2. the operators and the layers over the emulated kernels --------------------------------------------------------------------
def _graph_object(graph, N, num_src=None):
    from deepmetv2_amd.graph import BipartiteTable, EdgeList, NeighborTable
    if "nbr" in graph:
        return BipartiteTable(graph["nbr"], None, None, num_src) if num_src else NeighborTable(graph["nbr"], None, dense=False)
    tgt = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), graph["rowptr"].diff().long())
    return EdgeList(graph["src"], tgt, graph["rowptr"], N, num_src=num_src)


@pytest.fixture
def fake(monkeypatch):
    import pna_reference as pr
    fake_native.install(monkeypatch)
    wr.FakeNative().install(monkeypatch)
    pr.FakeKernels().install(monkeypatch)        # SAGEConv's aggr='max' is multi_aggregate


@pytest.mark.parametrize("kind", ["table", "list"])
def test_weighted_aggregate_over_emulated_kernels(fake, kind):
    import deepmetv2_amd as dm
    x, w, g_out, graph, pos, Nt = wr.kernel_case(kind, 5, 3)
    gr = _graph_object(graph, Nt)
    xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = dm.weighted_aggregate(xx, gr, ww.view(Nt, 3) if kind == "table" else ww)
    ref, count, _b = wr.forward(x, w, *pos, Nt)
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)
    out.backward(g_out)
    torch.testing.assert_close(xx.grad.double(), wr.grad_x(g_out, w, *pos, Nt)[0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ww.grad.double(), wr.grad_w(g_out, x, *pos)[0], rtol=1e-5, atol=1e-5)
    mean = dm.weighted_aggregate(x, gr, w, reduce="mean")
    torch.testing.assert_close(mean.double(), ref / count.clamp(min=1).view(-1, 1), rtol=1e-5, atol=1e-5)
    assert torch.equal(dm.weighted_aggregate(x, gr), dm.weighted_aggregate(x, gr, torch.ones_like(w), reduce="add"))
    # a gradient nobody needs is not asked of the kernels
    from deepmetv2_amd import _native
    asked = []
    real = _native._weighted_sum_bwd
    _native._weighted_sum_bwd = lambda *a: (asked.append(a[-2:]), real(*a))[1]
    try:
        dm.weighted_aggregate(x.clone().requires_grad_(True), gr, w).sum().backward()
        dm.weighted_aggregate(x, gr, w.clone().requires_grad_(True)).sum().backward()
        dm.weighted_aggregate(x.clone().requires_grad_(True), gr).sum().backward()
    finally:
        _native._weighted_sum_bwd = real
    assert asked == [(True, False), (False, True), (True, False)]


def test_spmm_returns_the_value_gradient_in_the_callers_order(fake):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(3)
    m, n, nnz, F = 9, 7, 40, 3
    index = torch.stack([torch.randint(0, m - 1, (nnz,), generator=g), torch.randint(0, n, (nnz,), generator=g)])
    index[:, 5] = index[:, 4]                    # a duplicate coordinate: the two values add
    value, matrix = torch.randn(nnz, generator=g), torch.randn(n, F, generator=g)
    v, mat = value.clone().requires_grad_(True), matrix.clone().requires_grad_(True)
    out = dm.spmm(index, v, m, n, mat)
    v64, m64 = value.double().requires_grad_(True), matrix.double().requires_grad_(True)
    dense = torch.zeros(m, n, dtype=torch.float64).index_put((index[0], index[1]), v64, accumulate=True)
    want = dense @ m64
    assert out.shape == (m, F) and bool((out[m - 1] == 0).all())
    torch.testing.assert_close(out.double(), want, rtol=1e-5, atol=1e-5)
    gg = torch.randn(m, F, generator=g)
    out.backward(gg)
    want.backward(gg.double())
    torch.testing.assert_close(v.grad.double(), v64.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(mat.grad.double(), m64.grad, rtol=1e-5, atol=1e-5)
    for bad in (dict(matrix=torch.randn(n + 1, F)), dict(value=torch.randn(nnz + 1)), dict(index=index[0])):
        a = {"index": index, "value": value, "matrix": matrix, **bad}
        with pytest.raises(ValueError):
            dm.spmm(a["index"], a["value"], m, n, a["matrix"])


@pytest.mark.parametrize("kind", ["table", "list"])
@pytest.mark.parametrize("name", list(wr.LAYERS))
def test_layer_over_emulated_kernels_matches_upstream(fake, name, kind):
    case = wr.layer_graph(kind)
    N, (tgt, src, valid) = case["N"], case["pos"]
    weighted = wr.LAYERS[name][4]
    ours, ref64, _ref32 = wr.build_layer(name)
    cin, cout = wr.LAYERS[name][2]
    g = torch.Generator().manual_seed(9)
    x, gout = torch.randn(N, cin, generator=g), torch.randn(N, cout, generator=g)
    w = case["w"] if weighted else None
    got = wr.layer_tensors(ours, x, (_graph_object(case["graph"], N),), w, gout, valid)
    want = wr.layer_tensors(ref64, x.double(), (src[valid], tgt[valid]), None if w is None else w.double()[valid], gout.double())
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_n, b) in zip(got, want):
        assert a is not None, n
        torch.testing.assert_close(a.double(), b, rtol=1e-4, atol=1e-4 * max(1.0, float(b.abs().max())), msg=lambda m, n=n: f"{n}: {m}")
    if name == "gcn_no_self_loops":          # an isolated node: the bias alone
        empty = torch.bincount(tgt[valid], minlength=N) == 0
        assert bool(empty.any()) and torch.equal(got[0][1][empty], ours.bias.detach().expand(int(empty.sum()), -1))


def test_pairs_and_bipartite_tables(fake):
    x_src, w, _g, graph, (tgt, src, valid), Nt = wr.kernel_case("table", 12, 16, 57)
    gr = _graph_object(graph, Nt, num_src=57)
    g = torch.Generator().manual_seed(10)
    x_dst, gout = torch.randn(Nt, 6, generator=g), torch.randn(Nt, wr.COUT, generator=g)
    for name, kwargs, weighted in (("graph_add", {}, True), ("sage_mean", {}, False), ("gin", {}, False)):
        ours, ref64, _ = wr.build_layer(name, channels=(12, 12) if name == "gin" else (12, 6))
        xd = torch.randn(Nt, 12, generator=g) if name == "gin" else x_dst
        ww = w.abs() if weighted else None
        got = wr.layer_tensors(ours, (x_src, xd), (gr,), ww, gout, valid)
        want = wr.layer_tensors(ref64, (x_src.double(), xd.double()), (src[valid], tgt[valid]),
                                None if ww is None else ww.double()[valid], gout.double())
        for (n, a), (_n, b) in zip(got, want):
            torch.testing.assert_close(a.double(), b, rtol=1e-4, atol=1e-4 * max(1.0, float(b.abs().max())), msg=lambda m, n=n: f"{name} {n}: {m}")


def test_shuffled_edge_index_with_weights_in_the_callers_order(fake):
    """A shuffled [2, E] tensor and edge_weight in its order against the grouped list and the grouped weights: the same
    bits forward, the weight gradient back in the caller's order."""
    case = wr.layer_graph("list")
    N, (tgt, src, valid) = case["N"], case["pos"]
    ours, _r64, _r32 = wr.build_layer("gcn")
    g = torch.Generator().manual_seed(11)
    x, gout = torch.randn(N, wr.CIN, generator=g), torch.randn(N, wr.COUT, generator=g)
    perm = torch.randperm(tgt.numel(), generator=g)
    ei = torch.stack([src[perm], tgt[perm]])
    a = wr.layer_tensors(ours, x, (_graph_object(case["graph"], N),), case["w"], gout)
    b = wr.layer_tensors(ours, x, (ei,), case["w"][perm], gout)
    for (n, p), (_n, q) in zip(a, b):
        if n == "g_w":           # edge e of the shuffled tensor is edge perm[e] of the grouped list
            torch.testing.assert_close(p[perm], q, rtol=1e-5, atol=1e-6)
        else:
            torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


def test_cached_keeps_the_normalisation(fake):
    import deepmetv2_amd as dm
    case = wr.layer_graph("table")
    N = case["N"]
    gr = _graph_object(case["graph"], N)
    torch.manual_seed(12)
    conv = dm.GCNConv(4, 4, cached=True)
    x = torch.randn(N, 4)
    a = conv(x, gr, case["w"])
    assert conv._cached_norm is not None
    b = conv(x, gr, case["w"])
    assert torch.equal(a, b)
    conv.reset_parameters()
    assert conv._cached_norm is None


# ---- 3. gcn_norm -----------------------------------------------------------------------------------------------------------------
def test_gcn_norm_on_written_loops_and_isolated_nodes(fake):
    import deepmetv2_amd as dm
    # node 0: a written loop of weight 0.5 and an edge from 1;  node 1: edges from 0 and 2;  node 2: two written loops
    # (both count: the stated deviation);  node 3: isolated;  node 4: an edge from 3
    src = torch.tensor([0, 1, 0, 2, 2, 2, 3], dtype=torch.int32)
    tgt = torch.tensor([0, 0, 1, 1, 2, 2, 4], dtype=torch.int32)
    w = torch.tensor([0.5, 2.0, 1.0, 3.0, 0.25, 0.75, 4.0])
    from deepmetv2_amd.graph import EdgeList, NeighborTable
    rowptr = torch.tensor([0, 2, 4, 6, 6, 7], dtype=torch.int32)
    edges = EdgeList(src, tgt, rowptr, 5)
    for improved, fill in ((False, 1.0), (True, 2.0)):
        ww = w.clone().requires_grad_(True)
        dinv, sw = dm.gcn_norm(edges, ww, 5, improved=improved)
        deg = torch.tensor([2.5, 4.0 + fill, 1.0, fill, 4.0 + fill])
        assert sw.tolist() == [0.0, fill, 0.0, fill, fill]
        torch.testing.assert_close(dinv, deg.pow(-0.5))
        dinv.sum().backward()
        torch.testing.assert_close(ww.grad, (-0.5 * deg.pow(-1.5))[tgt.long()])
    dinv, sw = dm.gcn_norm(edges, w, 5, add_self_loops=False)
    assert sw is None and dinv.tolist()[3] == 0.0                    # deg 0: 0, not inf
    torch.testing.assert_close(dinv, torch.tensor([2.5, 4.0, 1.0, 1.0, 4.0]).pow(-0.5) * torch.tensor([1, 1, 1, 0, 1.0]))
    ww = w.clone().requires_grad_(True)
    dm.gcn_norm(edges, ww, 5, add_self_loops=False)[0].sum().backward()
    assert bool(torch.isfinite(ww.grad).all())
    # the same graph as a table (a blank slot in between), unweighted: the degree is the entry count
    nbr = torch.tensor([[0, -1, 1], [0, 2, -1], [2, 2, -1], [-1, -1, -1], [-1, 3, -1]], dtype=torch.int32)
    dinv, sw = dm.gcn_norm(NeighborTable(nbr, None, dense=False), None, 5)
    assert sw.tolist() == [0.0, 1.0, 0.0, 1.0, 1.0]
    torch.testing.assert_close(dinv, torch.tensor([2.0, 3.0, 2.0, 1.0, 2.0]).pow(-0.5))
    with pytest.raises(ValueError):
        dm.gcn_norm(edges, None, 6)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(fake):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    from deepmetv2_amd.graph import BipartiteTable, NeighborTable
    mlp = torch.nn.Linear(4, 4)
    for make, who in ((lambda: dm.GCNConv(4, 4, edge_dim=3), "GCNConv"), (lambda: dm.GraphConv(4, 4, edge_dim=3), "GraphConv"),
                      (lambda: dm.SAGEConv(4, 4, edge_dim=3), "SAGEConv"), (lambda: dm.GINConv(mlp, edge_dim=3), "GINConv"),
                      (lambda: dm.GCNConv(4, 4, aggr="mean"), "GCNConv"), (lambda: dm.GraphConv(4, 4, aggr="max"), "GraphConv"),
                      (lambda: dm.SAGEConv(4, 4, aggr="lstm"), "SAGEConv"), (lambda: dm.GINConv(mlp, aggr="max"), "GINConv"),
                      (lambda: dm.GCNConv(4, 257), "GCNConv"), (lambda: dm.GraphConv(257, 258), "GraphConv"),
                      (lambda: dm.SAGEConv(257, 4), "SAGEConv")):
        with pytest.raises(ValueError, match=who):
            make()
    dm.GraphConv(300, 8), dm.GraphConv(8, 300)             # the narrower side is aggregated
    with pytest.raises(TypeError):
        dm.GCNConv(4, 4, flow="target_to_source")
    nbr = torch.tensor([[1, -1], [0, 2], [-1, -1]], dtype=torch.int32)
    table, x = NeighborTable(nbr, None, dense=False), torch.randn(3, 4)
    bip = BipartiteTable(nbr, None, None, 5)
    with pytest.raises(ValueError, match="GINConv"):
        dm.GINConv(torch.nn.Identity())(torch.randn(3, 257), table)
    with pytest.raises(ValueError, match="GCNConv"):
        dm.GCNConv(4, 4)((torch.randn(5, 4), x), bip)
    with pytest.raises(ValueError, match="GCNConv"):
        dm.GCNConv(4, 4)((x, x), torch.zeros(2, 0, dtype=torch.long))
    assert dm.GCNConv(4, 4, normalize=False)((torch.randn(5, 4), x), bip).shape == (3, 4)
    with pytest.raises(ValueError, match="GraphConv"):
        dm.GraphConv(4, 4)(x, bip)                          # a BipartiteTable needs a pair
    with pytest.raises(ValueError, match="SAGEConv"):
        dm.SAGEConv(4, 4)((x, x), table)                    # a pair goes with a BipartiteTable
    with pytest.raises(ValueError, match="GraphConv"):
        dm.GraphConv(4, 4)(torch.randn(4, 4), table)        # rows
    with pytest.raises(TypeError):
        dm.GraphConv(4, 4)(x, [[0], [1]])
    with pytest.raises(TypeError):
        dm.GraphConv(4, 4)(x, table, [1.0] * 6)
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(ValueError, match="GraphConv"):
        dm.GraphConv(4, 4)(x, ei, torch.ones(4))
    with pytest.raises(ValueError):
        dm.weighted_aggregate(x, table, torch.ones(5))
    with pytest.raises(ValueError):
        dm.weighted_aggregate(x, table, reduce="max")
    with pytest.raises(ValueError):
        dm.weighted_aggregate(torch.randn(3, 257), table)
    with pytest.raises(ValueError):
        dm.weighted_aggregate(torch.randn(4, 4), table)
    with pytest.raises(TypeError):
        dm.weighted_aggregate(x, "no graph")
    with pytest.raises(TypeError):
        dm.weighted_aggregate(x.half(), table)              # fp16 outside fp16 autocast
    with pytest.raises(ValueError):
        dm.weighted_aggregate(x, NeighborTable(nbr, None, dense=False, cnt=torch.tensor([1, 2, 0], dtype=torch.int32)).edge_list(),
                              torch.ones(7))
    for bad in (dict(x=torch.randn(6)), dict(x=torch.randn(6, 257)), dict(ns=5), dict(width=65), dict(width=0), dict(nt=-1),
                dict(w=torch.ones(23))):
        a = {"x": torch.randn(6, 8), "w": None, "nt": 6, "ns": 6, "width": 4, **bad}
        with pytest.raises(ValueError):
            _native.weighted_sum_check_shapes(a["x"], a["w"], a["nt"], a["ns"], a["width"])
    assert _native.WEIGHTED_SUM_MAX_F == 256


def test_cpu_tensors_are_refused_by_the_wrappers():
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import NeighborTable
    nbr = torch.tensor([[1, -1], [0, 0]], dtype=torch.int32)
    with pytest.raises(RuntimeError):            # no CPU fallback
        dm.weighted_aggregate(torch.randn(2, 4), NeighborTable(nbr, None, dense=False))


def test_exports():
    import deepmetv2_amd as dm
    for name in ("GCNConv", "GraphConv", "SAGEConv", "GINConv", "gcn_norm", "weighted_aggregate", "spmm"):
        assert name in dm.__all__ and hasattr(dm, name) and name in dm.__doc__
    assert sorted(dm.GCNConv(3, 5).state_dict()) == ["bias", "lin.weight"]
    assert sorted(dm.GraphConv(3, 5).state_dict()) == ["lin_rel.bias", "lin_rel.weight", "lin_root.weight"]
    assert sorted(dm.SAGEConv(3, 5, project=True).state_dict()) == ["lin.bias", "lin.weight", "lin_l.bias", "lin_l.weight", "lin_r.weight"]
    assert sorted(dm.GINConv(torch.nn.Linear(3, 5)).state_dict()) == ["eps", "nn.bias", "nn.weight"]
    assert [n for n, _ in dm.GINConv(torch.nn.Linear(3, 5), train_eps=True).named_parameters()][0] == "eps"
    assert not any(n == "eps" for n, _ in dm.GINConv(torch.nn.Linear(3, 5)).named_parameters())


# ---- 5. the C entries refuse bad arguments before any device work ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def test_abi_entries_refuse_bad_arguments_before_any_device_work(lib):
    p = 64        # any non-NULL address: a refused call never reads it

    def fwd(x=p, w=p, idx=p, rowptr=None, Nt=5, Ns=5, E=0, width=4, F=8, out=p, count=p):
        return lib.dmet_weighted_sum_fwd_f32(x, w, idx, rowptr, Nt, Ns, E, width, F, out, count, None)

    def bwd(x=p, w=p, g_out=p, idx=p, rowptr=None, tgt=None, rev_ptr=p, rev_pos=p, Nt=5, Ns=5, E=0, width=4, F=8, g_x=p,
            g_w=p):
        return lib.dmet_weighted_sum_bwd_f32(x, w, g_out, idx, rowptr, tgt, rev_ptr, rev_pos, Nt, Ns, E, width, F, g_x, g_w,
                                             None)

    for call in (fwd, bwd):
        for bad in (dict(F=0), dict(F=257), dict(width=-1), dict(width=65), dict(Nt=-1), dict(Ns=-1), dict(width=0, E=-1),
                    dict(width=0, E=3), dict(x=None), dict(idx=None)):
            assert call(**bad) == -22, (call.__name__, bad)
            assert b"dmet_weighted_sum" in lib.dmet_last_error()
    assert fwd(out=None) == -22
    assert bwd(g_x=None, g_w=None) == -22 and bwd(g_out=None) == -22 and bwd(rev_ptr=None) == -22 and bwd(rev_pos=None) == -22
    assert bwd(width=0, E=3, rowptr=p, tgt=None) == -22                      # a list needs tgt in the backward
    assert bwd(Nt=0, g_x=None, g_w=None) == -22                              # ... also on an empty problem
    # empty problems are no-ops; what a request does not need may be NULL
    assert fwd(Nt=0) == 0 and fwd(Nt=0, F=256, width=0) == 0 and bwd(Nt=0, Ns=0) == 0 and bwd(Nt=0, Ns=0, g_x=None) == 0

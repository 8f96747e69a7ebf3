"""PointNetConv without a GPU: the float64 reference against a triple loop, gradcheck and upstream's composed formula; the
argument errors (raised from shapes, before any device is asked for); -EINVAL through the library; and, for every case of
tests/test_gpu_pointnet.py, a seed without fragile elements over a brute-force float64 graph."""
import os
import shutil

import pytest
import torch

import pointnet_cases as pc
import pointnet_reference as pr


def _small(seed, act, act2, self_loop, F=3, D=2, H1=5, H2=4, N=7, width=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, F, generator=g, dtype=torch.float64) if F else None
    pos = torch.randn(N, D, generator=g, dtype=torch.float64)
    W1 = torch.randn(H1, F + D, generator=g, dtype=torch.float64)
    b1 = torch.randn(H1, generator=g, dtype=torch.float64)
    W2 = torch.randn(H2, H1, generator=g, dtype=torch.float64)
    b2 = torch.randn(H2, generator=g, dtype=torch.float64)
    nbr = torch.randint(-1, N, (N, width), generator=g)
    nbr[2] = -1                              # a row without an entry
    nbr[3, 0] = 3                            # a written self loop
    nbr[4, 1] = N + 5                        # an id outside the sources: an empty slot
    return x, pos, W1, b1, W2, b2, nbr, pr.entries_from_table(nbr, N, None, self_loop)


@pytest.mark.parametrize("act,act2,self_loop", [("relu", False, False), ("elu", True, True), ("relu", True, True),
                                                ("elu", False, False)])
def test_reference_equals_the_triple_loop(act, act2, self_loop):
    x, pos, W1, b1, W2, b2, nbr, entries = _small(3, act, act2, self_loop)
    ref = pr.Reference(x, pos, pos, W1, b1, W2, b2, act, act2, entries, 7)
    out, win = pr.loops(x, pos, pos, W1, b1, W2, b2, act, act2, entries, 7)
    assert torch.allclose(ref.out, out, rtol=1e-12, atol=1e-12)
    assert torch.equal(ref.win, win)
    if not self_loop:
        assert bool((ref.out[2] == 0).all()) and bool((ref.win[2] == -1).all())     # the empty row
    else:
        assert bool((ref.win[2] == -2).all())                                        # only the added entry
        assert not bool(((entries[0] == entries[1]) & ~entries[3]).any())           # written self loops are gone
    assert ref.fragile >= 0 and bool((ref.bar_m >= 0).all())


def test_table_and_list_entries_agree():
    nbr = torch.tensor([[2, -1, 0], [1, 1, 9], [-1, -1, -1]])
    t, s, c, f = pr.entries_from_table(nbr, 3, None, True)
    # row 0: slots 0 and 2 hold 2 and 0 -> 0 is a self loop and goes, then the added entry
    assert (t.tolist(), s.tolist(), c.tolist(), f.tolist()) == ([0, 0, 1, 2], [2, 0, 1, 2], [0, -2, -2, -2],
                                                                [False, True, True, True])
    t2, s2, c2, f2 = pr.entries_from_list(torch.tensor([2, 0, 1, 1]), torch.tensor([0, 0, 1, 1]), 3, True)
    assert (t2.tolist(), s2.tolist(), c2.tolist()) == ([0, 0, 1, 2], [2, 0, 1, 2], [0, -2, -2, -2])
    t3, _s3, c3, _f3 = pr.entries_from_table(nbr, 3, torch.tensor([1, 2, 3]), False)
    assert (t3.tolist(), c3.tolist()) == ([0, 1, 1], [0, 0, 1])                     # slots at or beyond cnt are not read


class _RefFn(torch.autograd.Function):
    """The reference's forward with its explicit backward, so that gradcheck differentiates the forward numerically
    and compares with the backward as written."""

    @staticmethod
    def forward(ctx, x, ps, pd, W1, b1, W2, b2, entries, act, act2, Nt):
        ctx.ref = pr.Reference(x, ps, pd, W1, b1, W2, b2, act, act2, entries, Nt)
        return ctx.ref.out.clone()

    @staticmethod
    def backward(ctx, g):
        d = ctx.ref.backward(g)
        return d["x"], d["pos_src"], d["pos_dst"], d["W1"], d["b1"], d["W2"], d["b2"], None, None, None, None


def test_gradcheck_of_the_elu_form():
    g = torch.Generator().manual_seed(11)
    Ns, Nt, F, D, H1, H2 = 6, 4, 3, 2, 4, 3
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)
    x, ps, pd, W1, b1, W2, b2 = mk(Ns, F), mk(Ns, D), mk(Nt, D), mk(H1, F + D), mk(H1), mk(H2, H1), mk(H2)
    nbr = torch.tensor([[0, 3, -1], [5, 5, 1], [-1, -1, -1], [2, 4, 0]])
    entries = pr.entries_from_table(nbr, Ns)
    for act2 in (False, True):
        assert torch.autograd.gradcheck(lambda *a: _RefFn.apply(*a, entries, "elu", act2, Nt), (x, ps, pd, W1, b1, W2, b2),
                                        eps=1e-6, atol=1e-6)


def _upstream(x, pos_src, pos_dst, edge_index, local_nn, num_targets, add_self_loops):
    """PyG's PointNetConv.forward composed from torch ops, with the edge index rewritten as upstream rewrites it."""
    if add_self_loops:
        keep = edge_index[0] != edge_index[1]
        ids = torch.arange(num_targets)
        edge_index = torch.cat([edge_index[:, keep], torch.stack([ids, ids])], dim=1)
    j, i = edge_index[0], edge_index[1]
    msg = pos_src[j] - pos_dst[i]
    if x is not None:
        msg = torch.cat([x[j], msg], dim=1)
    msg = local_nn(msg)
    out = msg.new_zeros((num_targets, msg.shape[1]))
    return out.scatter_reduce(0, i.view(-1, 1).expand_as(msg), msg, "amax", include_self=False)


@pytest.mark.parametrize("self_loop", [False, True])
def test_reference_equals_the_upstream_formula(self_loop):
    g = torch.Generator().manual_seed(5)
    N, F, D, H1, H2 = 9, 4, 3, 6, 5
    x = torch.randn(N, F, generator=g, dtype=torch.float64, requires_grad=True)
    pos = torch.randn(N, D, generator=g, dtype=torch.float64, requires_grad=True)
    nn = torch.nn.Sequential(torch.nn.Linear(F + D, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2)).double()
    tgt = torch.sort(torch.randint(0, N - 1, (30,), generator=g)).values           # node N-1 has no written edge
    src = torch.randint(0, N, (30,), generator=g)
    ei = torch.stack([src, tgt])
    out = _upstream(x, pos, pos, ei, nn, N, self_loop)
    gout = torch.randn(N, H2, generator=g, dtype=torch.float64)
    out.backward(gout)
    ref = pr.Reference(x, pos, pos, nn[0].weight, nn[0].bias, nn[2].weight, nn[2].bias, "relu", False,
                       pr.entries_from_list(src, tgt, N, self_loop), N)
    assert torch.allclose(ref.out, out.detach(), rtol=1e-12, atol=1e-12)
    d = ref.backward(gout)
    assert torch.allclose(d["x"], x.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(d["pos_src"] + d["pos_dst"], pos.grad, rtol=1e-10, atol=1e-12)
    for name, p in (("W1", nn[0].weight), ("b1", nn[0].bias), ("W2", nn[2].weight), ("b2", nn[2].bias)):
        assert torch.allclose(d[name], p.grad, rtol=1e-10, atol=1e-12), name
    if not self_loop:
        assert bool((ref.out[N - 1] == 0).all())


@pytest.mark.parametrize("case", list(pc.CASES))
def test_every_gpu_case_finds_a_seed_without_fragile_elements(case):
    seed, _inp, entries, ref = pc.find_seed(case, lambda inp: pc.brute_entries(case, inp))
    assert 0 <= seed < pc.TRIES and ref.fragile == 0
    Ns, Nt = pc.sizes(case)
    assert ref.out.shape == (Nt, pc.CASES[case]["H2"])
    if case == "set abstraction":
        deg = torch.bincount(entries[0], minlength=Nt)
        assert deg[:10].tolist() == [16] * 10 and deg[10:].tolist() == [7, 7]        # event 2 has short rows
    if case == "empty events":
        assert bool((ref.win[3:] == -1).all()) and bool((ref.out[3:] == 0).all())     # event 1 has no source
    if case == "tile edges":
        assert torch.bincount(entries[0], minlength=Nt)[:4].tolist() == [15, 16, 17, 40]


# ---- argument errors ----------------------------------------------------------------------------------------------------
def _layer(F=3, D=2, H1=8, H2=16, **kw):
    import deepmetv2_amd as dm
    return dm.PointNetConv(torch.nn.Sequential(torch.nn.Linear(F + D, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2)), **kw)


def test_layer_follows_upstream_names():
    import deepmetv2_amd as dm
    g = torch.nn.Linear(16, 4)
    conv = _layer(global_nn=g)
    assert conv.aggr == "max" and conv.flow == "source_to_target" and conv.add_self_loops is True
    assert sorted(conv.state_dict()) == ["global_nn.bias", "global_nn.weight", "local_nn.0.bias", "local_nn.0.weight",
                                         "local_nn.2.bias", "local_nn.2.weight"]
    before = conv.local_nn[0].weight.clone()
    conv.reset_parameters()
    assert not torch.equal(before, conv.local_nn[0].weight)
    assert dm.PointConv is dm.PointNetConv
    assert dm.PointNetConv().local_nn is None
    with pytest.raises(ValueError, match="aggr"):
        _layer(aggr="min")
    with pytest.raises(ValueError, match="flow"):
        _layer(flow="sideways")
    with pytest.raises(TypeError, match="unexpected"):
        _layer(heads=2)


def test_forward_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import BipartiteTable
    x, pos, pos_d = torch.randn(6, 3), torch.randn(6, 2), torch.randn(4, 2)
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="add_self_loops=False"):
        _layer()((x, None), (pos, pos_d), ei)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        _layer()(x, pos.view(-1), ei)
    with pytest.raises(ValueError, match="beside pos"):
        _layer()(x[:5], pos, ei)
    with pytest.raises(TypeError, match="edge_index"):
        _layer()(x, pos, "graph")
    table = BipartiteTable(torch.zeros((4, 2), dtype=torch.int32), None, None, 6)
    with pytest.raises(ValueError, match="pair"):
        _layer(add_self_loops=False)(x, pos, table)
    with pytest.raises(ValueError, match="queries"):
        _layer(add_self_loops=False)(x, (pos, torch.randn(5, 2)), table)


def test_aggregate_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import BipartiteTable
    x, pos, pos_d = torch.randn(6, 3), torch.randn(6, 2), torch.randn(4, 2)
    table = BipartiteTable(torch.zeros((4, 2), dtype=torch.int32), None, None, 6)
    lin = lambda i, o: torch.nn.Linear(i, o)
    with pytest.raises(TypeError, match="graph must be"):
        dm.pointnet_aggregate(x, pos, pos_d, "graph", lin(5, 8), lin(8, 16))
    with pytest.raises(ValueError, match="act must be"):
        dm.pointnet_aggregate(x, pos, pos_d, table, lin(5, 8), lin(8, 16), act="tanh")
    with pytest.raises(ValueError, match="one node set"):
        dm.pointnet_aggregate(x, pos, pos_d, table, lin(5, 8), lin(8, 16), self_loops=True)
    with pytest.raises(ValueError, match=r"W1 must be"):
        dm.pointnet_aggregate(x, pos, pos_d, table, lin(4, 8), lin(8, 16))
    with pytest.raises(ValueError, match="unsupported widths"):
        dm.pointnet_aggregate(x, pos, pos_d, table, lin(5, 8), lin(8, 24))
    with pytest.raises(ValueError, match="unsupported widths"):
        dm.pointnet_aggregate(x, pos, pos_d, table, lin(5, 129), lin(129, 16))
    with pytest.raises(ValueError, match="unsupported widths"):
        dm.pointnet_aggregate(None, torch.randn(6, 9), torch.randn(4, 9), table, lin(9, 8), lin(8, 16))
    with pytest.raises(ValueError, match="target rows"):
        dm.pointnet_aggregate(x, pos, torch.randn(5, 2), table, lin(5, 8), lin(8, 16))
    with pytest.raises(ValueError, match="x_src must be"):
        dm.pointnet_aggregate(x[:5], pos, pos_d, table, lin(5, 8), lin(8, 16))
    with pytest.raises(TypeError, match="float32"):
        dm.pointnet_aggregate(x, pos, pos_d, table, lin(5, 8).double(), lin(8, 16))
    wide = BipartiteTable(torch.zeros((4, 1025), dtype=torch.int32), None, None, 6)
    with pytest.raises(ValueError, match="width"):
        dm.pointnet_aggregate(x, pos, pos_d, wide, lin(5, 8), lin(8, 16))
    with pytest.raises(RuntimeError, match="non-GPU"):      # past the shape checks: there is no CPU path
        dm.pointnet_aggregate(x, pos, pos_d, table, lin(5, 8), lin(8, 16))


def test_route_selection_needs_no_device():
    from deepmetv2_amd.pointnet import _as_fused_local_nn
    S, L = torch.nn.Sequential, torch.nn.Linear
    assert _as_fused_local_nn(S(L(5, 8), torch.nn.ReLU(), L(8, 16)))[2:] == ("relu", False)
    assert _as_fused_local_nn(S(L(5, 8), torch.nn.ELU(), L(8, 16), torch.nn.ELU()))[2:] == ("elu", True)
    assert _as_fused_local_nn(S(L(5, 8), torch.nn.ELU(), L(8, 16), torch.nn.ReLU())) is None
    assert _as_fused_local_nn(S(L(5, 8), torch.nn.ELU(alpha=0.5), L(8, 16))) is None
    assert _as_fused_local_nn(S(L(5, 8), torch.nn.ReLU(), L(8, 8), torch.nn.ReLU(), L(8, 16))) is None
    assert _as_fused_local_nn(S(L(5, 8), torch.nn.BatchNorm1d(8), L(8, 16))) is None
    assert _as_fused_local_nn(None) is None and _as_fused_local_nn(L(5, 8)) is None


# ---- the library ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def _fwd(lib, Nt=10, Ns=10, E=0, width=4, F=3, D=2, H1=8, H2=16, act=0, act2=0, self_loop=0, rowptr=None, null=None):
    p = 64      # any non-null address: never touched
    args = dict(x=p, ps=p, pd=p, idx=p, rowptr=rowptr, cnt=None, W1=p, b1=p, W2=p, b2=p, a=p, b=p, s=p, out=p, win=p, ws=p)
    if null:
        args[null] = None
    return lib.dmet_pointnet_fwd_f32(args["x"], args["ps"], args["pd"], args["idx"], args["rowptr"], args["cnt"], Nt, Ns, E,
                                     width, F, D, args["W1"], args["b1"], H1, args["W2"], args["b2"], H2, act, act2, self_loop,
                                     args["a"], args["b"], args["s"], args["out"], args["win"], args["ws"], 1 << 30, None)


def _bwd(lib, Nt=10, Ns=10, E=0, width=4, F=3, D=2, H1=8, H2=16, act=0, act2=0, self_loop=0, rowptr=None, null=()):
    p = 64
    names = ("a", "b", "s", "out", "win", "g_out", "idx", "rowptr", "tgt", "cnt", "rev_ptr", "rev_pos", "W1", "W2", "g_a",
             "g_b", "g_s", "g_x", "g_ps", "g_pd", "g_W2", "g_b2", "ws")
    a = {n: p for n in names}
    a["rowptr"], a["cnt"] = rowptr, None
    for n in null:
        a[n] = None
    return lib.dmet_pointnet_bwd_f32(a["a"], a["b"], a["s"], a["out"], a["win"], a["g_out"], a["idx"], a["rowptr"], a["tgt"],
                                     a["cnt"], a["rev_ptr"], a["rev_pos"], Nt, Ns, E, width, F, D, a["W1"], H1, a["W2"], H2,
                                     act, act2, self_loop, a["g_a"], a["g_b"], a["g_s"], a["g_x"], a["g_ps"], a["g_pd"],
                                     a["g_W2"], a["g_b2"], a["ws"], 1 << 30, None)


def test_supported_and_workspace(lib):
    for F, D, H1, H2, ok in ((0, 1, 1, 16, 1), (128, 8, 128, 128, 1), (32, 2, 64, 64, 1), (129, 2, 8, 16, 0),
                             (3, 0, 8, 16, 0), (3, 9, 8, 16, 0), (3, 2, 0, 16, 0), (3, 2, 129, 16, 0), (3, 2, 8, 48, 0),
                             (-1, 2, 8, 16, 0)):
        assert lib.dmet_pointnet_supported(F, D, H1, H2) == ok, (F, D, H1, H2)
        assert (lib.dmet_pointnet_workspace_bytes(F, D, H1, H2) > 0) == bool(ok)
        from deepmetv2_amd import _native
        assert _native.pointnet_widths_supported(F, D, H1, H2) == bool(ok)


def test_einval_through_the_library(lib):
    """Bad arguments come back as -EINVAL with a message, before any device work (the pointers are never touched)."""
    for call, name in ((_fwd, b"dmet_pointnet_fwd_f32"), (_bwd, b"dmet_pointnet_bwd_f32")):
        for kw, word in ((dict(H2=24), b"H2=24"), (dict(F=129), b"F=129"), (dict(D=0), b"D=0"), (dict(H1=200), b"H1=200"),
                         (dict(Nt=-1), b"Nt=-1"), (dict(Ns=-3), b"Ns=-3"), (dict(width=0), b"width=0"),
                         (dict(width=1025), b"width=1025"), (dict(act=2), b"act"), (dict(self_loop=1, Ns=9), b"self_loop"),
                         (dict(rowptr=64, E=-1), b"E=-1")):
            assert call(lib, **kw) == -22, (name, kw)
            assert word in lib.dmet_last_error() and name in lib.dmet_last_error(), (kw, lib.dmet_last_error())
    for null in ("pd", "W1", "W2", "out", "win", "b", "idx", "ps", "a", "x", "ws"):
        assert _fwd(lib, null=null) == -22, null
        assert b"null" in lib.dmet_last_error() or b"workspace" in lib.dmet_last_error()
    assert _fwd(lib, self_loop=1, null="s") == -22
    for null in ("b", "out", "win", "g_out", "W1", "W2", "idx", "a", "rev_ptr", "rev_pos", "g_a", "g_b", "ws"):
        assert _bwd(lib, null=(null,)) == -22, null
    assert _bwd(lib, self_loop=1, null=("g_s",)) == -22
    assert _bwd(lib, rowptr=64, E=5, null=("tgt",)) == -22
    # empty problems are no-ops: no target in the forward; no target and no source in the backward
    assert _fwd(lib, Nt=0, Ns=5) == 0
    assert _bwd(lib, Nt=0, Ns=0, null=("g_W2", "g_b2")) == 0


def test_names_are_exported():
    import deepmetv2_amd as dm
    for name in ("PointNetConv", "PointConv", "pointnet_aggregate"):
        assert name in dm.__all__ and callable(getattr(dm, name))

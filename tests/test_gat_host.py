"""GATConv / GATv2Conv without a GPU: the float64 reference of tests/gat_reference.py against a plain per-node loop, the
layers' parameters under PyG's names, every argument error, and the check that a float32 run of the reference stays
inside half of each bar tests/test_gpu_gat.py holds the kernels to, on every input that file uses."""
import math
import os
import shutil

import pytest
import torch

import gat_reference as gr

# 12 nodes: a node without an edge (11), written self loops (0, 4, 4 twice), a node whose only edge is its loop (10)
TGT12 = torch.tensor([0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 4, 4, 4, 5, 6, 7, 7, 8, 9, 9, 10])
SRC12 = torch.tensor([0, 3, 7, 2, 2, 9, 1, 5, 6, 8, 4, 4, 0, 3, 3, 1, 9, 2, 7, 5, 10])


def _loop_reference(mode, xl, a, b, tgt, src, slope, self_loops):
    """The formulas node by node, head by head, entry by entry, in Python floats."""
    Nt = (a if mode == gr.V2 else b).shape[0]
    H, C = xl.shape[1], xl.shape[2]
    out = torch.zeros(Nt, H, C, dtype=torch.float64)
    for i in range(Nt):
        nb = [int(j) for t, j in zip(tgt.tolist(), src.tolist()) if t == i and not (self_loops and j == i)]
        if self_loops:
            nb.append(i)
        for h in range(H):
            scores = []
            for j in nb:
                if mode == gr.V2:
                    s = 0.0
                    for c in range(C):
                        t = float(xl[j, h, c]) + float(a[i, h, c])
                        s += float(b[h, c]) * (t if t > 0 else slope * t)
                else:
                    t = float(a[j, h]) + float(b[i, h])
                    s = t if t > 0 else slope * t
                scores.append(s)
            if not scores:
                continue
            top = max(scores)
            w = [math.exp(s - top) for s in scores]
            for j, wj in zip(nb, w):
                out[i, h] += wj / sum(w) * xl[j, h].double()
    return out


@pytest.mark.parametrize("mode", [gr.V1, gr.V2])
@pytest.mark.parametrize("self_loops", [False, True])
def test_reference_equals_the_per_node_loop(mode, self_loops):
    xl, a, b = (t.double() for t in gr.inputs(mode, 12, 12, 2, 3, seed=1))
    tgt, src = gr.with_self_loops(TGT12, SRC12, 12) if self_loops else (TGT12, SRC12)
    out, alpha, bar = gr.run(mode, xl, a, b, tgt, src, 0.2)
    want = _loop_reference(mode, xl, a, b, TGT12, SRC12, 0.2, self_loops)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    sums = torch.zeros(12, 2, dtype=torch.float64).index_add(0, tgt, alpha)
    deg = torch.bincount(tgt, minlength=12)
    torch.testing.assert_close(sums, (deg > 0).double().view(-1, 1).expand(-1, 2), rtol=1e-12, atol=1e-12)
    if self_loops:
        assert torch.equal(out[11], xl[11]) and torch.equal(out[10], xl[10])       # nothing but the added loop
        assert int((tgt == src).sum()) == 12
    else:
        assert bool((out[11] == 0).all()) and float(bar[11]) == 0.0


def test_the_slope_at_zero_is_torchs():
    """t == 0 takes the slope in the backward, as torch.nn.functional.leaky_relu: g_xr of an entry with t == 0."""
    xl = torch.zeros(2, 1, 1, dtype=torch.float64)
    xr = torch.zeros(1, 1, 1, dtype=torch.float64, requires_grad=True)
    xl[1] = 1.0
    att = torch.ones(1, 1, dtype=torch.float64)
    out, _alpha, _bar = gr.gatv2(xl, xr, att, torch.tensor([0, 0]), torch.tensor([0, 1]), 0.25)
    out.sum().backward()
    # alpha = softmax(0, 1); g_s = alpha (xl_j - out); g_xr = g_s_0 * 0.25 + g_s_1 * 1
    a1 = math.exp(1) / (1 + math.exp(1))
    o = a1
    want = (1 - a1) * (0 - o) * 0.25 + a1 * (1 - o) * 1.0
    assert abs(float(xr.grad) - want) < 1e-12


V2_KEYS = {"att": (1, 3, 6), "lin_l.weight": (18, 10), "lin_l.bias": (18,), "lin_r.weight": (18, 10), "lin_r.bias": (18,)}
V1_KEYS = {"att_src": (1, 3, 6), "att_dst": (1, 3, 6), "lin.weight": (18, 10)}


@pytest.mark.parametrize("name", list(gr.MODULE_CASES))
def test_module_parameters_are_pygs(name):
    import deepmetv2_amd as dm
    cls, in_channels, opts = gr.MODULE_CASES[name]
    conv = (dm.GATv2Conv if cls == "v2" else dm.GATConv)(in_channels, 6, heads=3, **opts)
    ref = gr.ref_module(name)
    shapes = {n: tuple(v.shape) for n, v in conv.state_dict().items()}
    assert shapes == {n: tuple(v.shape) for n, v in ref.state_dict().items()}
    width = 18 if opts.get("concat", True) else 6
    pair = not isinstance(in_channels, int)
    in_src, in_dst = in_channels if pair else (in_channels, in_channels)
    want = dict(V2_KEYS if cls == "v2" else V1_KEYS)
    if cls == "v2":
        want["lin_l.weight"], want["lin_r.weight"] = (18, in_src), (18, in_dst)
    elif pair:
        del want["lin.weight"]
        want["lin_src.weight"], want["lin_dst.weight"] = (18, in_src), (18, in_dst)
    if opts.get("bias", True):
        want["bias"] = (width,)
    if opts.get("residual"):
        want["res.weight"] = (width, in_dst)
    assert shapes == want
    if opts.get("share_weights"):
        assert conv.lin_r is conv.lin_l
    if conv.bias is not None:
        assert bool((conv.bias == 0).all())
    for n, p in conv.named_parameters():
        if n.startswith("att") or n.endswith("weight"):       # glorot: uniform within sqrt(6 / (fan_in + fan_out))
            lim = math.sqrt(6.0 / (p.shape[-2] + p.shape[-1]))
            top = float(p.detach().abs().max())
            assert 0.5 * lim < top <= lim, n
    # strict loading in both directions
    conv.load_state_dict({n: v.float() for n, v in ref.state_dict().items()}, strict=True)
    ref.load_state_dict({n: v.double() for n, v in conv.state_dict().items()}, strict=True)
    assert conv.heads == 3 and conv.out_channels == 6 and conv.dropout == 0.0 and conv.edge_dim is None
    assert conv.add_self_loops == opts["add_self_loops"]


def test_constructor_limits():
    import deepmetv2_amd as dm
    for cls in (dm.GATConv, dm.GATv2Conv):
        for bad in (dict(dropout=0.1), dict(edge_dim=4), dict(heads=17), dict(heads=0), dict(out_channels=65),
                    dict(out_channels=0), dict(heads=8, out_channels=33), dict(heads=2.0), dict(negative_slope=-0.1),
                    dict(negative_slope=float("nan"))):
            kw = dict(in_channels=8, out_channels=8)
            kw.update(bad)
            with pytest.raises(ValueError):
                cls(**kw)
        with pytest.raises(ValueError, match="add_self_loops=False"):
            cls((8, 6), 8)
        with pytest.raises(TypeError):
            cls(8, 8, aggr="max")
        cls(8, 64, heads=4)       # the limits themselves
        cls(8, 16, heads=16)
        cls((8, 6), 8, add_self_loops=False)
    with pytest.raises(ValueError, match="share_weights"):
        dm.GATv2Conv((8, 6), 8, add_self_loops=False, share_weights=True)
    with pytest.raises(TypeError):
        dm.GATConv(8, 8, share_weights=True)


NBR7 = torch.tensor([[0, 1, 2], [1, 0, -1], [2, 6, 5], [3, -1, -1], [4, 3, 2], [5, 4, 6], [6, 5, 0]], dtype=torch.int32)
XY = torch.tensor([[0, 6, 2], [1, -1, -1], [5, 4, 3]], dtype=torch.int32)


def _table(nbr):
    import deepmetv2_amd as dm
    return dm.NeighborTable(nbr, torch.tensor([0, nbr.shape[0]]), dense=False)


def test_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import EdgeList
    table = _table(NBR7)
    xy = dm.BipartiteTable(XY, torch.tensor([0, 7]), torch.tensor([0, 3]), 7)
    tgt, src, _pos = gr.table_entries(NBR7, 7)
    rowptr = torch.zeros(8, dtype=torch.int32)
    rowptr[1:] = torch.bincount(tgt, minlength=7).cumsum(0)
    edges = EdgeList(src.int(), tgt.int(), rowptr, 7)
    counted = dm.NeighborTable(NBR7, torch.tensor([0, 7]), dense=False, cnt=torch.full((7,), 2, dtype=torch.int32))
    r = torch.randn
    # v2
    xl, xr, att = gr.inputs(gr.V2, 7, 7, 2, 3, seed=3)
    for match, args in (("C=65", (r(7, 1, 65), r(7, 1, 65), r(1, 65), table)),
                        ("H=17", (r(7, 17, 2), r(7, 17, 2), r(17, 2), table)),
                        ("H\\*C=264", (r(7, 8, 33), r(7, 8, 33), r(8, 33), table)),
                        ("k=65", (xl, xr, att, _table(torch.zeros(7, 65, dtype=torch.int32)))),
                        ("xl must be", (xl.flatten(1), xr, att, table)),
                        ("xr must be", (xl, xr[:, :1], att, table)),
                        ("att must be", (xl, xr, att[:1], table)),
                        ("target rows", (xl, xr[:6], att, table)),
                        ("sources", (xl[:6], xr, att, table)),
                        ("counted", (xl, xr, att, counted)),
                        ("target rows", (xl, xr, att, xy)),
                        ("sources", (xl[:6], xr[:3], att, xy)),
                        ("sources", (xl[:5], xr, att, edges))):
        with pytest.raises(ValueError, match=match):
            dm.gat_aggregate(*args)
    with pytest.raises(ValueError, match="negative_slope"):
        dm.gat_aggregate(xl, xr, att, table, negative_slope=-1.0)
    with pytest.raises(ValueError, match="negative_slope"):
        dm.gat_aggregate(xl, xr, att, table, negative_slope=float("inf"))
    with pytest.raises(ValueError, match="self_loops=False"):
        dm.gat_aggregate(xl, xr[:3], att, xy, self_loops=True)
    with pytest.raises(ValueError, match="self_loops=False"):
        dm.gat_aggregate(xl, xr[:3], att, EdgeList(src.int() % 3, tgt.int() % 3, rowptr[:4], 3, num_src=7), self_loops=True)
    with pytest.raises(TypeError):
        dm.gat_aggregate(xl, xr, att, NBR7)
    with pytest.raises(TypeError):
        dm.gat_aggregate(xl.double(), xr, att, table)
    with pytest.raises(TypeError):
        dm.gat_aggregate(xl.half(), xr, att, table)          # fp16 outside fp16 autocast stays an error
    # v1
    xl, s_src, s_dst = gr.inputs(gr.V1, 7, 7, 2, 3, seed=4)
    for match, args in (("C=65", (r(7, 1, 65), r(7, 1), r(7, 1), table)),
                        ("H=17", (r(7, 17, 2), r(7, 17), r(7, 17), table)),
                        ("k=65", (xl, s_src, s_dst, _table(torch.zeros(7, 65, dtype=torch.int32)))),
                        ("s_src must be", (xl, s_src[:, :1], s_dst, table)),
                        ("s_src must be", (xl, s_src[:6], s_dst, table)),
                        ("s_dst must be", (xl, s_src, s_dst.unsqueeze(-1), table)),
                        ("target rows", (xl, s_src, s_dst[:6], table)),
                        ("counted", (xl, s_src, s_dst, counted)),
                        ("target rows", (xl, s_src, s_dst, xy)),
                        ("sources", (xl[:5], s_src[:5], s_dst, edges))):
        with pytest.raises(ValueError, match=match):
            dm.gat_v1_aggregate(*args)
    with pytest.raises(ValueError, match="self_loops=False"):
        dm.gat_v1_aggregate(xl, s_src, s_dst[:3], xy, self_loops=True)
    with pytest.raises(TypeError):
        dm.gat_v1_aggregate(xl, s_src, s_dst, NBR7)
    # well-formed arguments get as far as the device check: there is no CPU implementation
    xl2, xr, att = gr.inputs(gr.V2, 7, 7, 2, 3, seed=3)
    for graph, n in ((table, 7), (xy, 3), (edges, 7)):
        for loops in (False, True) if graph is not xy else (False,):
            with pytest.raises(RuntimeError, match="non-GPU"):
                dm.gat_aggregate(xl2, xr[:n], att, graph, self_loops=loops)
            with pytest.raises(RuntimeError, match="non-GPU"):
                dm.gat_v1_aggregate(xl, s_src, s_dst[:n], graph, self_loops=loops)


@pytest.mark.parametrize("cls", ["GATConv", "GATv2Conv"])
def test_forward_errors_on_cpu_tensors(cls):
    import deepmetv2_amd as dm
    table = _table(NBR7)
    xy = dm.BipartiteTable(XY, torch.tensor([0, 7]), torch.tensor([0, 3]), 7)
    make = getattr(dm, cls)
    conv, loops = make(4, 3, heads=2, add_self_loops=False), make(4, 3, heads=2)
    x = torch.randn(7, 4)
    with pytest.raises(ValueError, match="pair"):
        conv((x, x[:3]), table)
    with pytest.raises(ValueError, match="pair"):
        conv(x, xy)
    with pytest.raises(ValueError, match="pair"):
        conv((x, x, x), table)
    with pytest.raises(TypeError):
        conv(x, [[0, 1], [1, 0]])
    with pytest.raises(TypeError, match="int64"):
        conv(x, torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="\\[N, F\\]"):
        conv(x.view(7, 2, 2), table)
    with pytest.raises(ValueError, match="add_self_loops=False"):
        loops((x, x[:3]), xy)
    with pytest.raises(ValueError, match="add_self_loops=False"):
        loops(x, xy)
    with pytest.raises(ValueError, match="loop=True.*add_self_loops=False"):
        loops(x, table, return_attention_weights=True)
    for layer in (conv, loops):
        with pytest.raises(RuntimeError, match="non-GPU"):
            layer(x, table)
    assert "PyG is not installed" in make.__doc__ and "unpinned" in make.__doc__


# ---- the bars of tests/test_gpu_gat.py are reachable: a float32 run of the reference stays inside half of each ---------------------
def _half_bar_check(mode, case, what):
    tgt, src, N = gr.host_entries(case)
    if case["self_loops"]:
        tgt, src = gr.with_self_loops(tgt, src, N)
    xl, a, b = gr.inputs(mode, N, N, case["H"], case["C"], case["seed"], case["kind"])
    g = torch.randn(N, case["H"], case["C"], generator=torch.Generator().manual_seed(5))
    res = {}
    for dt in (torch.float32, torch.float64):
        ins = [t.detach().clone().to(dt).requires_grad_(True) for t in (xl, a, b)]
        out, alpha, bar = gr.run(mode, *ins, tgt, src, case["slope"])
        out.backward(g.to(dt))
        res[dt] = (out.detach(), alpha.detach(), bar, [t.grad for t in ins])
    o32, a32, _b32, g32 = res[torch.float32]
    o64, a64, bar, g64 = res[torch.float64]
    assert bool(torch.isfinite(o32).all())
    gr.assert_output_bar(o32, o64, bar, what, frac=0.5)
    torch.testing.assert_close(a32.double(), a64, rtol=0.5e-4, atol=0.5e-6)
    scale = gr.term_scale(mode, xl, a, b, tgt, src, case["slope"], g) if gr.cancelling(case) else None
    names = ("g_xl", "g_xr", "g_att") if mode == gr.V2 else ("g_xl", "g_s_src", "g_s_dst")
    target_side = "g_xr" if mode == gr.V2 else "g_s_dst"
    for name, x, ref in zip(names, g32, g64):
        gr.assert_grad_bar(x, ref, f"{what}: {name}", frac=0.5, scale=scale if name == target_side else None)


@pytest.mark.parametrize("mode", [gr.V1, gr.V2])
@pytest.mark.parametrize("name", list(gr.OPERATOR_CASES))
def test_the_bars_are_reachable_on_the_operator_cases(name, mode):
    _half_bar_check(mode, gr.OPERATOR_CASES[name], f"{name}, v{mode}")


@pytest.mark.parametrize("name", list(gr.MODULE_CASES))
def test_the_bars_are_reachable_on_the_module_cases(name):
    x, ei, _ns, _nd = gr.module_inputs(name)
    loops = gr.MODULE_CASES[name][2]["add_self_loops"]
    ref = gr.ref_module(name)
    pair = isinstance(x, tuple)
    res = {}
    for dt in (torch.float32, torch.float64):
        mod = gr.ref_module(name).to(dt)
        mod.load_state_dict({n: v.float().to(dt) for n, v in ref.state_dict().items()})       # the fp32-rounded parameters
        xs = tuple(t.detach().clone().to(dt).requires_grad_(True) for t in (x if pair else (x,)))
        out = mod(xs if pair else xs[0], ei[1], ei[0], add_self_loops=loops)
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(6))
        out.backward(g.to(dt))
        res[dt] = [("out", out.detach())] + [(f"gx{n}", t.grad) for n, t in enumerate(xs)] \
            + [(n, p.grad) for n, p in mod.named_parameters()]
    for (name32, a), (_n, b) in zip(res[torch.float32], res[torch.float64]):
        gr.assert_grad_bar(a, b, f"{name}: {name32}", frac=0.5)


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

    def fwd(mode=2, xl=p, xr=p, att=p, s_src=p, s_dst=p, slope=0.2, loops=0, idx=p, rowptr=None, Nt=5, Ns=5, E=0, width=4,
            H=2, C=8, out=p, lse=p):
        return lib.dmet_gat_fwd_f32(mode, xl, xr, att, s_src, s_dst, slope, loops, idx, rowptr, Nt, Ns, E, width, H, C, out,
                                    lse, None, None)

    def bwd(mode=2, xl=p, xr=p, att=p, s_src=p, s_dst=p, slope=0.2, loops=0, idx=p, rowptr=None, tgt=None, Nt=5, Ns=5, E=0,
            width=4, H=2, C=8, work=p, self_work=p, g_xl=p, g_xr=p, g_rows=p, g_ssrc=p, g_sdst=p):
        return lib.dmet_gat_bwd_f32(mode, xl, xr, att, s_src, s_dst, slope, loops, p, p, p, idx, rowptr, tgt, p, p, Nt, Ns, E,
                                    width, H, C, work, work, self_work, self_work, g_xl, g_xr, g_rows, g_ssrc, g_sdst, None)

    for call in (fwd, bwd):
        for bad in (dict(C=0), dict(C=65), dict(H=0), dict(H=17), dict(H=8, C=33), dict(H=1, C=257), dict(width=0), dict(width=65),
                    dict(Nt=-1), dict(Ns=-1), dict(rowptr=p, E=-1), dict(xl=None), dict(idx=None), dict(mode=0), dict(mode=3),
                    dict(slope=-0.5), dict(slope=float("nan")), dict(slope=float("inf")), dict(loops=1, Ns=6), dict(loops=2),
                    dict(xr=None), dict(att=None), dict(mode=1, s_src=None), dict(mode=1, s_dst=None)):
            assert call(**bad) == -22, (call.__name__, bad)
            assert b"dmet_gat" in lib.dmet_last_error()
    assert fwd(out=None) == -22 and fwd(lse=None) == -22
    assert bwd(g_xl=None) == -22 and bwd(g_xr=None) == -22 and bwd(g_rows=None) == -22 and bwd(work=None) == -22
    assert bwd(mode=1, g_ssrc=None) == -22 and bwd(mode=1, g_sdst=None) == -22 and bwd(rowptr=p, E=3, tgt=None) == -22
    assert bwd(loops=1, self_work=None) == -22
    assert fwd(H=16, C=16, Nt=0) == 0 and fwd(H=4, C=64, Nt=0) == 0        # the limits themselves; no target: a no-op
    assert fwd(mode=1, Nt=0, xr=None, att=None) == 0 and bwd(Nt=0, Ns=0) == 0
    assert [lib.dmet_gat_supported(H, C) for H, C in ((1, 1), (4, 64), (16, 16), (0, 8), (17, 1), (1, 65), (8, 33))] \
        == [1, 1, 1, 0, 0, 0, 0]

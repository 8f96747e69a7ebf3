"""Attention without a GPU: the float64 reference against a plain triple loop and gradcheck, a float32 run of the
reference on the GPU tests' inputs inside half of their bars, TransformerConv's parameters against PyG's published names,
the constructor limits, and the argument errors (raised from shapes, before any device is asked for; -EINVAL from the ABI
entries before any device work)."""
import math
import os
import shutil

import pytest
import torch

import attention_reference as ar

NBR7 = torch.tensor([[0, 1, 2, 3],
                     [1, 0, -1, -1],
                     [2, -1, 4, 6],
                     [-1, 3, 5, -1],
                     [-1, -1, -1, -1],
                     [5, 5, 0, 6],
                     [6, 2, 1, 0]], dtype=torch.int32)
XY = torch.tensor([[6, 0, -1], [-1, -1, -1], [3, 3, 5]], dtype=torch.int32)      # 3 queries over 7 candidates


def _loops(q, k, v, nbr):
    Nt, H, C = q.shape
    out = torch.zeros(Nt, H, C, dtype=torch.float64)
    alpha = torch.zeros(Nt, nbr.shape[1], H, dtype=torch.float64)
    bar = torch.zeros(Nt, dtype=torch.float64)
    for i in range(Nt):
        slots = [t for t in range(nbr.shape[1]) if int(nbr[i, t]) >= 0]
        for t in slots:
            bar[i] = max(float(bar[i]), float(v[int(nbr[i, t])].abs().max()))
        for h in range(H):
            s = [sum(float(q[i, h, c]) * float(k[int(nbr[i, t]), h, c]) for c in range(C)) / math.sqrt(C) for t in slots]
            if not s:
                continue
            m = max(s)
            e = [math.exp(x - m) for x in s]
            for t, x in zip(slots, e):
                alpha[i, t, h] = x / sum(e)
                for c in range(C):
                    out[i, h, c] += x / sum(e) * float(v[int(nbr[i, t]), h, c])
    return out, alpha, bar


@pytest.mark.parametrize("nbr, nt", [(NBR7, 7), (XY, 3)], ids=["one set, an empty row", "two sets, an empty row"])
def test_reference_equals_the_triple_loop(nbr, nt):
    q, k, v = (t.double() for t in ar.qkv(nt, 7, 2, 3, seed=1))
    tgt, src, pos = ar.table_entries(nbr, 7)
    out, alpha, bar = ar.attention(q, k, v, tgt, src)
    l_out, l_alpha, l_bar = _loops(q, k, v, nbr)
    torch.testing.assert_close(out, l_out, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(ar.table_alpha(alpha, pos, nt, nbr.shape[1]), l_alpha, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(bar, l_bar, rtol=0, atol=0)
    empty = 4 if nt == 7 else 1
    assert bool((out[empty] == 0).all()) and float(bar[empty]) == 0.0


def test_reference_gradcheck():
    q, k, v = (t.double().requires_grad_(True) for t in ar.qkv(7, 7, 2, 3, seed=2))
    tgt, src, _pos = ar.table_entries(NBR7, 7)
    assert torch.autograd.gradcheck(lambda a, b, c: ar.attention(a, b, c, tgt, src)[0], (q, k, v), eps=1e-6, atol=1e-6)
    ref = ar.RefTransformerConv(4, 3, heads=2, beta=True)
    x = torch.randn(7, 4, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a: ref(a, tgt, src), (x,), eps=1e-6, atol=1e-6)


def _float32_inside_half_the_bars(q, k, v, tgt, src, what, cancelling_g_q=False):
    g = torch.randn(q.shape, generator=torch.Generator().manual_seed(5))
    res = {}
    for dt in (torch.float64, torch.float32):
        qq, kk, vv = (t.to(dt).requires_grad_(True) for t in (q, k, v))
        out, _alpha, bar = ar.attention(qq, kk, vv, tgt, src)
        out.backward(g.to(dt))
        res[dt] = (out.detach(), bar, qq.grad, kk.grad, vv.grad)
    r64, r32 = res[torch.float64], res[torch.float32]
    ar.assert_output_bar(r32[0], r64[0], r64[1], what, frac=0.5)
    for name, a, b in zip(("g_q", "g_k", "g_v"), r32[2:], r64[2:]):
        scale = ar.g_q_term_scale(q, k, v, tgt, src, g) if cancelling_g_q and name == "g_q" else None
        ar.assert_grad_bar(a, b, f"{what}: {name}", frac=0.5, scale=scale)


@pytest.mark.parametrize("case", list(ar.KNN_CASES))
def test_the_bar_is_reachable_on_the_knn_cases(case):
    sizes, H, C, k = ar.KNN_CASES[case]
    N = sum(sizes)
    q, kk, v = ar.qkv(N, N, H, C, seed=len(case))
    tgt, src, _pos = ar.table_entries(ar.host_knn(ar.coords(N, len(case)), k, sizes), N)
    _float32_inside_half_the_bars(q, kk, v, tgt, src, case)


def test_the_bar_is_reachable_on_the_other_gpu_inputs():
    for C in ar.CHANNEL_WIDTHS:
        q, k, v = ar.qkv(49, 49, 2, C, seed=C)
        tgt, src, _pos = ar.table_entries(ar.host_knn(ar.coords(49, C), 8, [40, 9]), 49)
        _float32_inside_half_the_bars(q, k, v, tgt, src, f"C={C}")
    ei, N = ar.degree_edge_index()
    q, k, v = ar.qkv(N, N, 2, 16, seed=31)
    _float32_inside_half_the_bars(q, k, v, ei[1], ei[0], "in-degrees")
    q, k, v = ar.exact_score_inputs(N)
    _float32_inside_half_the_bars(q, k, v, ei[1], ei[0], "exact scores", cancelling_g_q=True)


OPTIONS = {
    "concat": dict(concat=True, beta=False, root_weight=True),
    "mean": dict(concat=False, beta=False, root_weight=True),
    "beta": dict(concat=True, beta=True, root_weight=True),
    "no root": dict(concat=False, beta=True, root_weight=False),
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_module_parameters_are_pygs(name):
    import deepmetv2_amd as dm
    opt = OPTIONS[name]
    conv = dm.TransformerConv((11, 9), 5, heads=3, **opt)
    width = 15 if opt["concat"] else 5
    want = {"lin_key.weight": (15, 11), "lin_key.bias": (15,), "lin_query.weight": (15, 9), "lin_query.bias": (15,),
            "lin_value.weight": (15, 11), "lin_value.bias": (15,)}
    if opt["root_weight"]:
        want.update({"lin_skip.weight": (width, 9), "lin_skip.bias": (width,)})
        if opt["beta"]:
            want["lin_beta.weight"] = (1, 3 * width)
    assert {n: tuple(v.shape) for n, v in conv.state_dict().items()} == want
    assert (conv.heads, conv.out_channels, conv.concat, conv.beta) == (3, 5, opt["concat"], opt["beta"] and opt["root_weight"])
    ref = ar.RefTransformerConv((11, 9), 5, heads=3, **opt)
    conv.load_state_dict({n: v.float() for n, v in ref.state_dict().items()})      # strict: the same keys
    assert "lin_skip.bias" not in dm.TransformerConv(4, 4, bias=False).state_dict()
    assert repr(dm.TransformerConv(4, 5, heads=2)) == "TransformerConv(4, 5, heads=2)"


def test_constructor_limits():
    import deepmetv2_amd as dm
    for bad in (dict(heads=0), dict(heads=17), dict(out_channels=0), dict(out_channels=65), dict(heads=8, out_channels=33),
                dict(heads=2.0), dict(dropout=0.1), dict(edge_dim=4)):
        kw = dict(out_channels=16, heads=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            dm.TransformerConv(8, **kw)
    with pytest.raises(TypeError):
        dm.TransformerConv(8, 8, aggr="max")
    dm.TransformerConv(8, 64, heads=4)       # the limits themselves
    dm.TransformerConv(8, 16, heads=16)


def _table(nbr):
    import deepmetv2_amd as dm
    return dm.NeighborTable(nbr, torch.tensor([0, nbr.shape[0]]), dense=False)


def test_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import EdgeList
    q, k, v = ar.qkv(7, 7, 2, 3, seed=3)
    table = _table(NBR7)
    with pytest.raises(ValueError, match="C=65"):
        dm.attention_aggregate(torch.randn(7, 1, 65), torch.randn(7, 1, 65), torch.randn(7, 1, 65), table)
    with pytest.raises(ValueError, match="H=17"):
        dm.attention_aggregate(torch.randn(7, 17, 2), torch.randn(7, 17, 2), torch.randn(7, 17, 2), table)
    with pytest.raises(ValueError, match="H\\*C=264"):
        dm.attention_aggregate(torch.randn(7, 8, 33), torch.randn(7, 8, 33), torch.randn(7, 8, 33), table)
    with pytest.raises(ValueError, match="k=65"):
        dm.attention_aggregate(q, k, v, _table(torch.zeros(7, 65, dtype=torch.int32)))
    with pytest.raises(ValueError, match="3-D"):
        dm.attention_aggregate(q.flatten(1), k, v, table)
    with pytest.raises(ValueError, match="heads"):
        dm.attention_aggregate(q, k[:, :1], v, table)
    with pytest.raises(ValueError, match="rows"):
        dm.attention_aggregate(q, k, v[:6], table)
    with pytest.raises(ValueError, match="target rows"):
        dm.attention_aggregate(q[:6], k, v, table)
    with pytest.raises(ValueError, match="counted"):
        dm.attention_aggregate(q, k, v, dm.NeighborTable(NBR7, torch.tensor([0, 7]), dense=False,
                                                         cnt=torch.full((7,), 2, dtype=torch.int32)))
    with pytest.raises(TypeError):
        dm.attention_aggregate(q, k, v, NBR7)
    xy = dm.BipartiteTable(XY, torch.tensor([0, 7]), torch.tensor([0, 3]), 7)
    with pytest.raises(ValueError, match="target rows"):
        dm.attention_aggregate(q, k, v, xy)
    with pytest.raises(ValueError, match="sources"):
        dm.attention_aggregate(q[:3], k[:6], v[:6], xy)
    tgt, src, _pos = ar.table_entries(NBR7, 7)
    rowptr = torch.zeros(8, dtype=torch.int32)
    rowptr[1:] = torch.bincount(tgt, minlength=7).cumsum(0)
    edges = EdgeList(src.int(), tgt.int(), rowptr, 7)
    with pytest.raises(ValueError, match="sources"):
        dm.attention_aggregate(q, k[:5], v[:5], edges)
    # well-formed arguments get as far as the device check: there is no CPU implementation
    for graph, qq in ((table, q), (xy, q[:3]), (edges, q)):
        with pytest.raises(RuntimeError, match="non-GPU"):
            dm.attention_aggregate(qq, k, v, graph)
    conv = dm.TransformerConv(4, 3, heads=2)
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

    def fwd(q=p, k=p, v=p, idx=p, rowptr=None, Nt=5, Ns=5, E=0, width=4, H=2, C=8, out=p, lse=p):
        return lib.dmet_attention_fwd_f32(q, k, v, idx, rowptr, Nt, Ns, E, width, H, C, out, lse, None, None)

    def bwd(q=p, idx=p, rowptr=None, tgt=None, Nt=5, Ns=5, E=0, width=4, H=2, C=8, g_q=p, g_k=p, work=p):
        return lib.dmet_attention_bwd_f32(q, p, p, p, p, p, idx, rowptr, tgt, p, p, Nt, Ns, E, width, H, C, work, work,
                                          g_q, g_k, p, None)

    for call in (fwd, bwd):
        for bad in (dict(C=0), dict(C=65), dict(H=0), dict(H=17), dict(H=8, C=33), dict(H=1, C=257), dict(width=0), dict(width=65),
                    dict(Nt=-1), dict(Ns=-1), dict(rowptr=p, E=-1), dict(q=None), dict(idx=None)):
            assert call(**bad) == -22, (call.__name__, bad)
            assert b"dmet_attention" in lib.dmet_last_error()
    assert fwd(out=None) == -22 and fwd(lse=None) == -22 and fwd(k=None) == -22
    assert bwd(g_q=None) == -22 and bwd(g_k=None) == -22 and bwd(work=None) == -22 and bwd(rowptr=p, E=3, tgt=None) == -22
    assert fwd(H=16, C=16, Nt=0) == 0 and fwd(H=4, C=64, Nt=0) == 0        # the limits themselves; no target: a no-op
    assert [lib.dmet_attention_supported(H, C) for H, C in ((1, 1), (4, 64), (16, 16), (0, 8), (17, 1), (1, 65), (8, 33))] \
        == [1, 1, 1, 0, 0, 0, 0]

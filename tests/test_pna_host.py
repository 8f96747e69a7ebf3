"""PNAConv, DegreeScalerAggregation, multi_aggregate and scatter_std without a GPU: the float64 reference of
tests/pna_reference.py against an independent composition, the scalers from a hand-computed histogram, the layers'
refusals and route choice, the A_i + B_j split against the per-edge formula, and the fp32 simulations that show the
bounds of tests/test_gpu_pna.py are reachable by the kernels' chains (at most half of each) and not by a variance
formed from two fp32 means."""
import math
import os
import shutil

import numpy as np
import pytest
import torch

import fake_native
import pna_cases as pc
import pna_reference as pr


# ---- 1. the reference against a second composition -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,data", [("table", "normal"), ("table", "ints"), ("list", "normal"), ("table", "const_rows")])
def test_reference_equals_scatter_reduce_composition(kind, data):
    x, _graph, (tgt, src, valid), Nt, ref = pc.case(kind, 5, data, 1, k=17)
    pos = torch.nonzero(valid).view(-1)
    i, j = tgt[pos], src[pos]
    xs = x.double()[j]
    idx = i.view(-1, 1).expand_as(xs)
    zeros = torch.zeros(Nt, 5, dtype=torch.float64)
    n = torch.bincount(i, minlength=Nt)
    assert torch.equal(n, ref["count"])
    s = zeros.index_add(0, i, xs)
    torch.testing.assert_close(s, ref["sum"], rtol=1e-13, atol=1e-13)
    mean = s / n.clamp(min=1).view(-1, 1)
    torch.testing.assert_close(mean, ref["mean"], rtol=1e-13, atol=1e-13)
    var = zeros.index_add(0, i, (xs - mean[i]) ** 2) / n.clamp(min=1).view(-1, 1)
    torch.testing.assert_close(var, ref["var"], rtol=1e-11, atol=1e-18)
    for name, how in (("min", "amin"), ("max", "amax")):
        val = zeros.scatter_reduce(0, idx, xs, how, include_self=False)
        assert torch.equal(val, ref[name])
        # the lowest position among the winners
        won = torch.where(xs == val[i], pos.view(-1, 1).expand_as(xs), torch.full_like(idx, 2 ** 40))
        arg = torch.full((Nt, 5), 2 ** 40).scatter_reduce(0, idx, won, "amin", include_self=True)
        arg = torch.where(arg == 2 ** 40, torch.full_like(arg, -1), arg)
        assert torch.equal(arg, ref["arg" + name])
    assert bool((ref["count"] == 0).any()) and bool((ref["count"] == 1).any())
    empty = ref["count"] == 0
    for name in pr.KINDS:
        assert bool((ref[name][empty] == 0).all())
    if data == "const_rows":
        assert bool((ref["var"] == 0).all()) and bool((ref["std"] == 0).all())
    if data == "ints":
        assert bool((ref["argmin"] != ref["argmax"])[ref["count"] > 1].any())


def test_reference_gradient_equals_autograd():
    aggrs = ("sum", "mean", "min", "max", "var", "std")
    x, _graph, (tgt, src, valid), Nt, ref = pc.case("list", 4, "normal", 2)
    g_out = pc.upstream_gradient(aggrs, Nt, 4, 1, 2).double()
    g = pr.layout(g_out, aggrs, 1)
    g_x, n_j = pr.grad(x, tgt, src, valid, ref, g)
    pos = torch.nonzero(valid).view(-1)
    xx = x.double().requires_grad_(True)
    msg = xx[src[pos]]
    outs = [pr.upstream_aggregate(msg, tgt[pos], Nt, a) for a in aggrs]      # var as mean(x^2) - mean(x)^2: float64 carries it
    for a, o in zip(aggrs, outs):
        torch.testing.assert_close(o.detach(), ref[a], rtol=1e-9, atol=1e-9)
    sum(float(1) * (o * g[a]).sum() for a, o in zip(aggrs, outs)).backward()
    torch.testing.assert_close(g_x, xx.grad, rtol=1e-8, atol=1e-8)
    assert n_j[-10:].tolist() == [0] * 10 and bool((g_x[-10:] == 0).all())       # sources without an outgoing edge


# ---- 2. scalers ----------------------------------------------------------------------------------------------------------
def test_scalers_from_a_hand_computed_histogram(monkeypatch):
    import deepmetv2_amd as dm
    deg = torch.tensor([1, 2, 0, 3])         # one node of in-degree 0, two of 1, three of 3: N = 6
    lin = (0 * 1 + 1 * 2 + 3 * 3) / 6
    log = (math.log(1) * 1 + math.log(2) * 2 + math.log(4) * 3) / 6
    scalers = ["identity", "amplification", "attenuation", "linear", "inverse_linear"]
    m = dm.DegreeScalerAggregation(["sum"], scalers, deg)
    assert math.isclose(float(m.avg_deg_lin), lin, rel_tol=1e-6) and math.isclose(float(m.avg_deg_log), log, rel_tol=1e-6)
    assert pr.avg_degrees(deg) == (m.init_avg_deg_lin, m.init_avg_deg_log)
    assert sorted(m.state_dict()) == ["avg_deg_lin", "avg_deg_log"] and not list(m.parameters())
    t = dm.DegreeScalerAggregation("mean", "linear", deg, train_norm=True)
    assert sorted(n for n, _ in t.named_parameters()) == ["avg_deg_lin", "avg_deg_log"]
    fac = m.factors(torch.tensor([0, 1, 3]))
    d = [1.0, 1.0, 3.0]                       # the degree is clamped to at least 1
    want = [[1.0, math.log(v + 1) / log, log / math.log(v + 1), v / lin, lin / v] for v in d]
    torch.testing.assert_close(fac, torch.tensor(want), rtol=1e-6, atol=0)
    for bad in (dict(aggr="median"), dict(scaler="cube"), dict(aggr=[]), dict(aggr=["sum", "sum"]), dict(scaler=[])):
        with pytest.raises(ValueError):
            dm.DegreeScalerAggregation(**{"aggr": "sum", "scaler": "identity", "deg": deg, **bad})
    # the module over the emulated kernels: scaler-major [n, S*A*F] as upstream composes it, an unsorted index
    fake_native.install(monkeypatch)
    pr.FakeKernels().install(monkeypatch)
    g = torch.Generator().manual_seed(3)
    x, index = torch.randn(40, 3, generator=g), torch.randint(0, 7, (40,), generator=g)
    index[index == 4] = 5                     # row 4 stays empty
    mod = dm.DegreeScalerAggregation(["mean", "max", "std"], scalers, deg)
    got = mod(x, index, dim_size=8)
    want = pr.upstream_degree_scaler(x.double(), index, 8, mod.aggr, scalers, lin, log)
    assert got.shape == (8, 5 * 3 * 3)
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-5)
    assert bool((got[4] == 0).all()) and bool((got[7] == 0).all())


# ---- 3. the layer: refusals, routes, names ----------------------------------------------------------------------------------
DEG = torch.tensor([2, 5, 9, 4, 1])


def test_refusals_and_limits():
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    ok = dict(in_channels=8, out_channels=8, aggregators=["mean"], scalers=["identity"], deg=DEG)
    for bad in (dict(edge_dim=3), dict(towers=3), dict(towers=0), dict(in_channels=9, towers=2, divide_input=True),
                dict(pre_layers=0), dict(aggregators=["median"]), dict(scalers=["square"]), dict(act="nope", pre_layers=2),
                dict(deg=torch.zeros(3))):
        with pytest.raises(ValueError):
            dm.PNAConv(**{**ok, **bad})
    conv = dm.PNAConv(**ok)
    with pytest.raises(ValueError):
        conv(torch.randn(5, 7), torch.zeros(2, 0, dtype=torch.long))
    with pytest.raises(TypeError):
        conv(torch.randn(5, 8), [[0], [1]])
    x = torch.randn(6, 8)
    for bad in (dict(aggrs=[]), dict(aggrs=["mean", "mean"]), dict(aggrs=["mode"]), dict(groups=3), dict(groups=0),
                dict(x=torch.randn(6, 257)), dict(x=torch.randn(6)), dict(ns=5), dict(width=65), dict(width=0)):
        a = {"x": x, "aggrs": ["mean"], "groups": 1, "nt": 6, "ns": 6, "width": 4, **bad}
        with pytest.raises(ValueError):
            _native.multi_aggr_check_shapes(a["x"], a["aggrs"], a["groups"], a["nt"], a["ns"], a["width"])
    assert _native.multi_aggr_code(["mean", "min", "max", "std"]) == 0x6432
    with pytest.raises(TypeError):
        dm.multi_aggregate(x, "no graph", ["sum"])
    with pytest.raises(RuntimeError):            # CPU tensors reach the wrapper and are refused there: no CPU fallback
        dm.scatter_std(torch.randn(5, 2), torch.tensor([0, 0, 1, 1, 1]))


def test_route_choice(monkeypatch):
    import deepmetv2_amd as dm
    x = torch.randn(4, 8)
    one = dm.PNAConv(8, 8, ["mean"], ["identity"], DEG)
    two = dm.PNAConv(8, 8, ["mean"], ["identity"], DEG, pre_layers=2)
    assert one.route(x) == "fused" and two.route(x) == "generic" and one.route(x.bfloat16()) == "generic"
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)       # what the layer asks on a ROCm device
    assert one.route(x) == "generic"
    monkeypatch.undo()
    monkeypatch.setenv("DMET_PNA", "0")
    assert one.route(x) == "generic"


def test_state_dict_names():
    import deepmetv2_amd as dm
    conv = dm.PNAConv(8, 12, ["mean", "std"], ["identity", "linear"], DEG, towers=2, pre_layers=2, post_layers=2,
                      train_norm=True)
    want = ["aggr_module.avg_deg_lin", "aggr_module.avg_deg_log", "lin.weight", "lin.bias"]
    for t in range(2):
        for nn in ("pre_nns", "post_nns"):
            want += [f"{nn}.{t}.{layer}.{p}" for layer in (0, 2) for p in ("weight", "bias")]
    assert sorted(conv.state_dict()) == sorted(want)
    assert conv.pre_nns[0][0].weight.shape == (8, 16) and conv.post_nns[1][0].weight.shape == (6, (2 * 2 + 1) * 8)
    assert conv.lin.weight.shape == (12, 12)
    ref = pr.UpstreamPNAConv(8, 12, ["mean", "std"], ["identity", "linear"], DEG, towers=2, pre_layers=2, post_layers=2,
                             train_norm=True)
    ref.load_state_dict(conv.state_dict())      # the restatement carries the same names and shapes


def _graph14():
    """14 nodes; node 13 has no incoming edge, node 12 no outgoing one, 3 -> 0 twice."""
    tgt = torch.tensor([0, 0, 0, 1, 2, 2, 3, 4, 4, 4, 4, 5, 6, 7, 8, 9, 10, 11, 12, 12, 5, 1])
    src = torch.tensor([3, 3, 7, 0, 1, 13, 2, 5, 6, 7, 8, 4, 0, 6, 9, 8, 11, 10, 0, 1, 13, 9])
    return torch.stack([src, tgt])


@pytest.mark.parametrize("towers,divide", [(1, False), (4, False), (4, True)])
def test_split_equals_the_per_edge_formula_in_float64(towers, divide):
    """A_i + B_j against pre_nn(cat[x_i, x_j]) aggregated per edge, all in float64, with a node of in-degree 0."""
    ei = _graph14()
    src, tgt = ei[0], ei[1]
    N, Fi = 14, (8 // towers if divide else 8)
    torch.manual_seed(4)
    ref = pr.UpstreamPNAConv(8, 8, list(pr.KINDS), ["identity"], DEG, towers=towers, divide_input=divide).double()
    x = torch.randn(N, 8, dtype=torch.float64)
    xt = x.view(N, towers, Fi) if divide else x.view(N, 1, Fi).repeat(1, towers, 1)
    h = torch.cat([xt[tgt], xt[src]], -1)
    msg = torch.stack([nn(h[:, t]) for t, nn in enumerate(ref.pre_nns)], 1)             # [E, T, F_in]
    W = torch.stack([nn[0].weight for nn in ref.pre_nns])
    b = torch.stack([nn[0].bias for nn in ref.pre_nns])
    a_rows = torch.einsum("ntf,tgf->ntg", xt, W[:, :, :Fi]) + b
    b_rows = torch.einsum("ntf,tgf->ntg", xt, W[:, :, Fi:])
    pos = (tgt, src, torch.ones_like(tgt, dtype=torch.bool))
    st = pr.stats(b_rows.reshape(N, -1).detach(), *pos, N)
    has = (st["count"] > 0).double().view(-1, 1)
    shift = {"sum": st["count"].double().view(-1, 1), "mean": has, "min": has, "max": has, "var": 0 * has, "std": 0 * has}
    for kind in pr.KINDS:
        want = pr.upstream_aggregate(msg, tgt, N, kind).reshape(N, -1).detach()
        got = st[kind] + shift[kind] * a_rows.reshape(N, -1).detach()
        torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9, msg=lambda m, k=kind: f"{k}: {m}")
        assert bool((got[13] == 0).all())


@pytest.mark.parametrize("kwargs", [dict(towers=1), dict(towers=4), dict(towers=4, divide_input=True), dict(pre_layers=2, towers=2),
                                    dict(towers=2, env="0")])
def test_layer_over_emulated_kernels_matches_upstream(monkeypatch, kwargs):
    """Both routes of the layer through the fp32 emulation of the kernels, outputs and every gradient against the float64
    restatement."""
    import deepmetv2_amd as dm
    kwargs = dict(kwargs)
    if kwargs.pop("env", None):
        monkeypatch.setenv("DMET_PNA", "0")
    fake_native.install(monkeypatch)
    pr.FakeKernels().install(monkeypatch)
    aggrs, scalers = ["mean", "min", "max", "std", "sum", "var"], ["identity", "amplification", "attenuation"]
    torch.manual_seed(5)
    conv = dm.PNAConv(8, 8, aggrs, scalers, DEG, **kwargs)
    ref = pr.UpstreamPNAConv(8, 8, aggrs, scalers, DEG, **kwargs).double()
    ref.load_state_dict(conv.state_dict())
    ei = _graph14()
    x = torch.randn(14, 8)
    xa, xb = x.clone().requires_grad_(True), x.double().requires_grad_(True)
    out, want = conv(xa, ei), ref(xb, ei)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(6))
    out.backward(g)
    want.backward(g.double())
    torch.testing.assert_close(out.double(), want, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(xa.grad.double(), xb.grad, rtol=1e-3, atol=1e-4)
    for (n, p), (_m, q) in zip(conv.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        torch.testing.assert_close(p.grad.double(), q.grad, rtol=1e-3, atol=1e-4 * max(1.0, float(q.grad.abs().max())),
                                   msg=lambda m, n=n: f"{n}: {m}")


# ---- 4. the bounds are reachable by the kernels' chains, and only by a centred variance -------------------------------------
def test_variance_chain_simulation():
    """n in 15..300, values 1000 + N(0,1): the centred two-pass fp32 chain stays under half of the variance bound, the
    one-pass form mean(x^2) - mean(x)^2 lands far outside it, in every trial."""
    rng = np.random.default_rng(7)
    worst_centred, best_one_pass = 0.0, math.inf
    for n in (15, 16, 17, 40, 64, 65, 150, 300):
        x = torch.from_numpy(1000.0 + rng.standard_normal((n, 8))).float()
        tgt, src, valid = torch.zeros(n, dtype=torch.long), torch.arange(n), torch.ones(n, dtype=torch.bool)
        ref = pr.stats(x, tgt, src, valid, 1)
        bound = pr.bounds(ref)["var"].numpy()
        two = pr.emulate_fwd(x.numpy(), tgt, src, valid, 1)["var"].astype(np.float64)
        one = pr.emulate_fwd(x.numpy(), tgt, src, valid, 1, one_pass=True)["var"].astype(np.float64)
        worst_centred = max(worst_centred, float((np.abs(two - ref["var"].numpy()) / bound).max()))
        best_one_pass = min(best_one_pass, float((np.abs(one - ref["var"].numpy()) / bound).max()))
    print(f"centred variance: worst error / bound {worst_centred:.3f}; one-pass form: best error / bound {best_one_pass:.0f}")
    assert worst_centred <= 0.5
    assert best_one_pass > 100.0


SIM = [("table", 5, "normal", 3), ("table", 4, "offset1000", 3), ("table", 4, "offset-50", 64), ("list", 5, "normal", 3),
       ("list", 3, "offset1000", 3), ("list", 3, "offset-50", 3), ("table", 5, "ints", 17), ("table", 4, "const_rows", 16)]


@pytest.mark.parametrize("kind,F,data,k", SIM)
def test_kernel_chain_simulation_stays_under_half_of_every_bound(kind, F, data, k):
    """The fp32 emulation of csrc/multi_aggr.hip's chains on the inputs of tests/test_gpu_pna.py against the float64
    reference: exact where the GPU test asks for equality, at most half of each bound elsewhere, g_x included."""
    aggrs = pr.KINDS
    x, _graph, pos, Nt, ref = pc.case(kind, F, data, 11, k=k)
    f = pr.emulate_fwd(x.numpy(), *pos, Nt)
    assert np.array_equal(f["count"], ref["count"].numpy())
    for name in ("min", "max", "argmin", "argmax"):
        assert np.array_equal(f[name].astype(np.float64), ref[name].double().numpy()), name
    b = pr.bounds(ref)
    for name in ("sum", "mean", "var", "std"):
        err = np.abs(f[name].astype(np.float64) - ref[name].numpy())
        lim = b[name].numpy()
        if name == "std":
            big = ref["var"].numpy() > 4e-5
            assert np.array_equal(f["std"][~big], np.zeros_like(f["std"][~big]))
            err, lim = err[big], lim[big]
        ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
        print(f"{kind} {data} {name}: emulated error / bound {ratio:.3f}")
        assert ratio <= 0.5, (name, ratio)
    if data in ("ints", "const_rows"):
        assert np.array_equal(f["sum"].astype(np.float64), ref["sum"].numpy())
    g_out = pc.upstream_gradient(aggrs, Nt, F, 1, 11)
    g = pr.layout(g_out, aggrs, 1)
    g_x = pr.emulate_bwd(x.numpy(), *pos, f, {a: t.numpy() for a, t in g.items()})
    g64 = {a: t.double() for a, t in g.items()}
    want, _n = pr.grad(x, *pos, ref, g64)
    lim = pr.grad_bound(x, *pos, ref, g64)
    ratio = float(((torch.from_numpy(g_x).double() - want).abs() / lim).max())
    print(f"{kind} {data} g_x: emulated error / bound {ratio:.3f}")
    assert ratio <= 0.5


# ---- 5. the C entries refuse bad arguments before any device work ------------------------------------------------------------
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

    def fwd(x=p, idx=p, rowptr=None, Nt=5, Ns=5, E=0, width=4, F=8, G=1, aggrs=0x6432, out=p, count=p, mean=p, var=p,
            amin=p, amax=p):
        return lib.dmet_multi_aggr_fwd_f32(x, idx, rowptr, Nt, Ns, E, width, F, G, aggrs, out, count, mean, var, amin, amax,
                                           None)

    def bwd(x=p, g_out=p, count=p, mean=p, var=p, amin=p, amax=p, tgt=None, rev_ptr=p, rev_pos=p, Nt=5, Ns=5, E=0, width=4,
            F=8, G=1, aggrs=0x6432, c0=p, c1=p, g_x=p):
        return lib.dmet_multi_aggr_bwd_f32(x, g_out, count, mean, var, amin, amax, tgt, rev_ptr, rev_pos, Nt, Ns, E, width,
                                           F, G, aggrs, c0, c1, g_x, None)

    for call in (fwd, bwd):
        for bad in (dict(F=0), dict(F=257), dict(G=0), dict(G=3), dict(width=-1), dict(width=65), dict(Nt=-1), dict(Ns=-1),
                    dict(width=0, E=-1), dict(aggrs=0), dict(aggrs=0x7), dict(aggrs=0x22), dict(aggrs=0x1234561),
                    dict(x=None), dict(mean=None), dict(var=None), dict(amin=None), dict(amax=None), dict(count=None)):
            assert call(**bad) == -22, (call.__name__, bad)
            assert b"dmet_multi_aggr" in lib.dmet_last_error()
    assert fwd(out=None) == -22 and fwd(idx=None) == -22 and fwd(width=0, E=3) == -22        # a list needs rowptr
    assert bwd(g_x=None) == -22 and bwd(c0=None) == -22 and bwd(c1=None) == -22 and bwd(g_out=None) == -22
    assert bwd(rev_pos=None) == -22 and bwd(width=0, E=3, tgt=None) == -22
    # empty problems are no-ops; what a request does not need may be NULL
    assert fwd(Nt=0) == 0 and fwd(Nt=0, F=256, G=4, aggrs=0x654321) == 0 and bwd(Ns=0) == 0 and bwd(Nt=0, Ns=0) == 0
    assert fwd(Nt=0, aggrs=0x21, mean=None, var=None, amin=None, amax=None) == 0

"""event_moments, event_normalize and GraphNorm / InstanceNorm / LayerNorm / PairNorm / GraphSizeNorm / MeanSubtractionNorm
without a GPU: the closed-form gradients of tests/event_norm_reference.py against float64 autograd, the fp32 emulation of
csrc/event_norm.hip's chains under half of every bound of tests/test_gpu_event_norm.py on that file's inputs, the layers
over the emulated kernels against their float64 restatements, state_dict keys, every refusal and the C entries' argument
checks."""
import os
import shutil

import pytest
import torch

import event_norm_reference as er
import fake_native


@pytest.fixture
def fake(monkeypatch):
    fake_native.install(monkeypatch)
    er.FakeKernels().install(monkeypatch)


SMALL = [0, 1, 2, 5, 0, 9, 3, 0]


# ---- 1. the closed-form gradients are the gradients ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["channel", "graph", "pair"])
def test_reference_gradients_equal_autograd(mode):
    g = torch.Generator().manual_seed(1)
    rowptr, N, F = er.rowptr_of(SMALL), sum(SMALL), 5
    x = (torch.randn(N, F, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    alpha = (0.7 + 0.3 * torch.randn(F, generator=g, dtype=torch.float64)) if mode == "channel" else torch.ones(F, dtype=torch.float64)
    alpha, w, b = (t.requires_grad_(True) for t in (alpha, 1 + 0.3 * torch.randn(F, generator=g, dtype=torch.float64),
                                                     torch.randn(F, generator=g, dtype=torch.float64)))
    gout = torch.randn(N, F, generator=g, dtype=torch.float64)
    y = er.normalize(x, rowptr, alpha, w, b, 1e-5, mode)
    y.backward(gout)
    g_x, g_alpha, g_w, g_b = er.normalize_grads(x.detach(), gout, rowptr, alpha.detach(), w.detach(), b.detach(), 1e-5, mode)
    torch.testing.assert_close(g_x, x.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(g_w, w.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(g_b, b.grad, rtol=1e-10, atol=1e-10)
    if mode == "channel":
        torch.testing.assert_close(g_alpha, alpha.grad, rtol=1e-10, atol=1e-10)


def test_reference_moments_gradient_equals_autograd():
    g = torch.Generator().manual_seed(2)
    rowptr, N, F = er.rowptr_of(SMALL), sum(SMALL), 4
    x = torch.randn(N, F, generator=g, dtype=torch.float64).requires_grad_(True)
    gm, gv = torch.randn(len(SMALL), F, generator=g, dtype=torch.float64), torch.randn(len(SMALL), F, generator=g, dtype=torch.float64)
    mean, var = er._stats(x, rowptr)
    ((mean * gm).sum() + (var * gv).sum()).backward()
    torch.testing.assert_close(er.moments_grad(x.detach(), gm, gv, rowptr), x.grad, rtol=1e-10, atol=1e-10)
    m64, v64, _bm, _bv = er.moments(x.detach(), rowptr)
    torch.testing.assert_close(m64, mean.detach()), torch.testing.assert_close(v64, var.detach())


# ---- 2. the bounds are reachable by the kernels' chains ----------------------------------------------------------------------
def _ratio(err, lim):
    assert bool((err[lim == 0] == 0).all())
    return float((err / lim.clamp(min=1e-300)).max())


@pytest.mark.parametrize("F", er.WIDTHS)
def test_kernel_chain_emulation_stays_under_half_of_every_bound(F):
    rowptr = er.rowptr_of(er.LENGTHS)
    for kind in ("gauss", "offset"):
        x = er.data(F, kind)
        mean, var, b_mean, b_var = er.moments(x, rowptr)
        for hint in er.HINTS:
            m, v = er.emulate_moments(x.numpy(), rowptr, hint)
            r_m = _ratio((torch.from_numpy(m).double() - mean).abs(), b_mean)
            r_v = _ratio((torch.from_numpy(v).double() - var).abs(), b_var)
            print(f"F={F} {kind} hint={hint}: emulated mean error / bound {r_m:.3f}, var {r_v:.3f}")
            assert r_m <= 0.5 and r_v <= 0.5, (kind, hint, r_m, r_v)
    x, g = er.data(F, "gauss"), er.data(F, "gauss", seed=1)
    mean, var, _bm, _bv = er.moments(x, rowptr)
    shift, scale = mean.float(), (1 / torch.sqrt(var + 1e-5)).float()
    s1, s2, b1, b2 = er.dots(g, x, rowptr, shift, scale)
    for hint in er.HINTS:
        a1, a2 = er.emulate_dots(g.numpy(), x.numpy(), rowptr, shift.numpy(), scale.numpy(), hint)
        r1 = _ratio((torch.from_numpy(a1).double() - s1).abs(), b1)
        r2 = _ratio((torch.from_numpy(a2).double() - s2).abs(), b2)
        print(f"F={F} hint={hint}: emulated s1 error / bound {r1:.3f}, s2 {r2:.3f}")
        assert r1 <= 0.5 and r2 <= 0.5, (hint, r1, r2)


def test_exact_data_gives_the_exact_mean_in_the_emulation():
    rowptr = er.rowptr_of(er.LENGTHS)
    x = er.data(5, "int")
    for hint in er.HINTS:
        m, v = er.emulate_moments(x.numpy(), rowptr, hint)
        for b, (lo, hi) in enumerate(er._spans(rowptr, x.shape[0])):
            want = (x[lo:hi].double().sum(0).float() / torch.tensor(float(max(hi - lo, 1)))) if hi > lo else torch.zeros(5)
            assert torch.equal(torch.from_numpy(m[b]), want)
            assert hi > lo or not v[b].any()


# ---- 3. the operators and the layers over the emulated kernels ------------------------------------------------------------------
def test_event_moments_over_emulated_kernels(fake):
    import deepmetv2_amd as dm
    lengths = SMALL
    rowptr, batch = er.rowptr_of(lengths), er.batch_of(lengths)
    x = er.data(5, "gauss", lengths)
    xx = x.clone().requires_grad_(True)
    mean, var, count = dm.event_moments(xx, batch, batch_size=len(lengths))
    m64, v64, _bm, _bv = er.moments(x, rowptr)
    assert count.tolist() == lengths
    torch.testing.assert_close(mean.double(), m64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(var.double(), v64, rtol=1e-5, atol=1e-6)
    g = torch.Generator().manual_seed(3)
    gm, gv = torch.randn(mean.shape, generator=g), torch.randn(var.shape, generator=g)
    ((mean * gm).sum() + (var * gv).sum()).backward()
    torch.testing.assert_close(xx.grad.double(), er.moments_grad(x.double(), gm.double(), gv.double(), rowptr), rtol=1e-5, atol=1e-6)
    # ptr wins over batch; neither: one event
    a = dm.event_moments(x, batch.flip(0), ptr=rowptr.long())
    assert torch.equal(a[0], mean.detach())
    one = dm.event_moments(x)
    torch.testing.assert_close(one[0].double(), x.double().mean(0, keepdim=True), rtol=1e-5, atol=1e-6)
    assert one[2].tolist() == [x.shape[0]]
    half = dm.event_moments(x.bfloat16(), batch, batch_size=len(lengths))
    assert half[0].dtype == torch.bfloat16 and half[1].dtype == torch.bfloat16


@pytest.mark.parametrize("mode", ["channel", "graph", "pair"])
def test_event_normalize_over_emulated_kernels(fake, mode):
    import deepmetv2_amd as dm
    lengths = SMALL + [70]
    rowptr, N, F = er.rowptr_of(lengths), sum(lengths), 6
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, F, generator=g) + 0.5
    alpha = 0.7 + 0.3 * torch.randn(F, generator=g) if mode == "channel" else None
    w, b, gout = 1 + 0.3 * torch.randn(F, generator=g), torch.randn(F, generator=g), torch.randn(N, F, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)] + ([alpha.clone().requires_grad_(True)] if mode == "channel" else [])
    y = dm.event_normalize(leaves[0], ptr=rowptr.long(), mean_scale=leaves[3] if mode == "channel" else None, weight=leaves[1],
                           bias=leaves[2], mode=mode)
    y.backward(gout)
    a64 = alpha.double() if mode == "channel" else torch.ones(F, dtype=torch.float64)
    want = er.normalize(x.double(), rowptr, a64, w.double(), b.double(), 1e-5, mode)
    g_x, g_alpha, g_w, g_b = er.normalize_grads(x.double(), gout.double(), rowptr, a64, w.double(), b.double(), 1e-5, mode)
    for name, got, ref in (("y", y.detach(), want), ("g_x", leaves[0].grad, g_x), ("g_w", leaves[1].grad, g_w),
                           ("g_b", leaves[2].grad, g_b)) + ((("g_alpha", leaves[3].grad, g_alpha),) if mode == "channel" else ()):
        # 1e-3: the gradient of a one-node event cancels to g w r (1 - alpha) eps r^2 from terms of size g w r
        torch.testing.assert_close(got.double(), ref, rtol=1e-3, atol=1e-3, msg=lambda m, name=name: f"{name}: {m}")
    # a gradient nobody needs is not computed
    xx = x.clone().requires_grad_(True)
    dm.event_normalize(xx, ptr=rowptr.long(), weight=w, bias=b, mode=mode).backward(gout)
    assert w.grad is None and b.grad is None and xx.grad is not None
    out = dm.event_normalize(x.bfloat16(), ptr=rowptr.long(), mode=mode)
    assert out.dtype == torch.bfloat16


@pytest.mark.parametrize("F", [3, 16])
@pytest.mark.parametrize("name", list(er.LAYERS))
def test_layer_over_emulated_kernels_matches_upstream(fake, name, F):
    lengths = SMALL + [70, 0]
    batch, B = er.batch_of(lengths), len(lengths)
    g = torch.Generator().manual_seed(5)
    x, gout = torch.randn(sum(lengths), F, generator=g) + 0.3, torch.randn(sum(lengths), F, generator=g)
    mod = er.build_layer(name, F)
    got = er.layer_tensors_ours(mod, x, batch, gout, B)
    want = er.layer_tensors_upstream(name, mod, x, batch, B, gout, torch.float64)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_n, b) in zip(got, want):
        assert a is not None, n
        torch.testing.assert_close(a.double(), b, rtol=1e-4, atol=1e-4 * max(1.0, float(b.abs().max())), msg=lambda m, n=n: f"{n}: {m}")


def test_layer_norm_node_mode_and_single_event(fake):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(6)
    x = torch.randn(40, 7, generator=g)
    node = dm.LayerNorm(7, mode="node")
    assert torch.equal(node(x), torch.nn.functional.layer_norm(x, (7,), node.weight, node.bias, 1e-5))
    graph = dm.LayerNorm(7)
    assert torch.equal(graph(x), graph(x, torch.zeros(40, dtype=torch.long)))
    assert torch.equal(dm.event_normalize(x), dm.event_normalize(x, ptr=torch.tensor([0, 40])))


def test_instance_norm_running_statistics(fake):
    import deepmetv2_amd as dm
    lengths = SMALL + [70]
    batch, B, F = er.batch_of(lengths), len(lengths), 4
    mod = dm.InstanceNorm(F, affine=True, track_running_stats=True, momentum=0.3)
    with torch.no_grad():
        mod.weight.copy_(torch.tensor([1.5, 0.5, -1.0, 2.0])), mod.bias.copy_(torch.tensor([0.1, -0.2, 0.3, 0.0]))
    rm, rv = torch.zeros(F, dtype=torch.float64), torch.ones(F, dtype=torch.float64)
    for step in range(2):
        x = er.data(F, "gauss", lengths, seed=step) + 2.0
        mod(x, batch, B)
        mean, _var, unbiased = er.up_instance_stats(x.double(), batch, B)
        rm, rv = 0.7 * rm + 0.3 * mean.mean(0), 0.7 * rv + 0.3 * unbiased.mean(0)
    torch.testing.assert_close(mod.running_mean.double(), rm, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(mod.running_var.double(), rv, rtol=1e-5, atol=1e-6)
    mod.eval()
    x = er.data(F, "gauss", lengths, seed=7)
    gout = er.data(F, "gauss", lengths, seed=8)
    got = er.layer_tensors_ours(mod, x, batch, gout, B)
    cfg = {"eps": mod.eps, "running": (rm, rv)}
    p = {n: t.detach().double().requires_grad_(True) for n, t in mod.named_parameters()}
    xx = x.double().requires_grad_(True)
    out = er.up_instance_norm(xx, batch, B, p, cfg)
    out.backward(gout.double())
    want = [("out", out.detach()), ("g_x", xx.grad), ("weight", p["weight"].grad), ("bias", p["bias"].grad)]
    for (n, a), (_n, b) in zip(got, want):
        torch.testing.assert_close(a.double(), b, rtol=1e-4, atol=1e-4, msg=lambda m, n=n: f"{n}: {m}")


def test_state_dict_keys_and_exports():
    import deepmetv2_amd as dm
    for name in ("GraphNorm", "InstanceNorm", "LayerNorm", "PairNorm", "GraphSizeNorm", "MeanSubtractionNorm", "event_moments",
                 "event_normalize"):
        assert name in dm.__all__ and hasattr(dm, name) and name in dm.__doc__
    assert sorted(dm.GraphNorm(3).state_dict()) == ["bias", "mean_scale", "weight"]
    assert sorted(dm.InstanceNorm(3).state_dict()) == []
    assert sorted(dm.InstanceNorm(3, affine=True, track_running_stats=True).state_dict()) == \
        ["bias", "num_batches_tracked", "running_mean", "running_var", "weight"]
    assert sorted(dm.LayerNorm(3).state_dict()) == ["bias", "weight"]
    assert sorted(dm.LayerNorm(3, affine=False).state_dict()) == []
    assert sorted(dm.PairNorm().state_dict()) == [] and sorted(dm.GraphSizeNorm().state_dict()) == []
    assert sorted(dm.MeanSubtractionNorm().state_dict()) == []
    gn = dm.GraphNorm(4)
    assert gn.weight.tolist() == [1.0] * 4 and gn.bias.tolist() == [0.0] * 4 and gn.mean_scale.tolist() == [1.0] * 4


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(fake):
    import deepmetv2_amd as dm
    x = torch.randn(6, 3)
    with pytest.raises(ValueError, match="sorted"):
        dm.GraphNorm(3)(x, torch.tensor([0, 1, 0, 1, 2, 2]))
    with pytest.raises(ValueError, match="sorted"):
        dm.event_moments(x, torch.tensor([0, 1, 0, 1, 2, 2]))
    with pytest.raises(ValueError, match=r"\[N, F\]"):
        dm.event_normalize(torch.randn(6))
    with pytest.raises(ValueError, match=r"\[N, F\]"):
        dm.LayerNorm(3)(torch.randn(2, 3, 3))
    with pytest.raises(ValueError, match="mode"):
        dm.event_normalize(x, mode="layer")
    with pytest.raises(ValueError, match="mode"):
        dm.LayerNorm(3, mode="batch")
    with pytest.raises(ValueError, match="batch values"):
        dm.InstanceNorm(3)(x, torch.tensor([0, 0, 1, 1, 2, 2]), batch_size=2)
    with pytest.raises(ValueError, match="batch values"):
        dm.event_normalize(x, torch.tensor([0, 0, 1, 1, 2, 2]), batch_size=2)
    with pytest.raises(ValueError, match="weight"):
        dm.event_normalize(x, weight=torch.ones(4))
    with pytest.raises(ValueError, match="mean_scale"):
        dm.event_normalize(x, mean_scale=torch.ones(3), mode="graph")
    with pytest.raises(ValueError):
        dm.event_moments(x, torch.tensor([0, 0, 1]))            # one batch entry per row
    with pytest.raises(TypeError):
        dm.event_moments(x.double())
    with pytest.raises(TypeError):
        dm.event_moments(x.long())


def test_cpu_tensors_are_refused_by_the_wrappers():
    import deepmetv2_amd as dm
    with pytest.raises(RuntimeError):            # no CPU fallback
        dm.GraphNorm(3)(torch.randn(4, 3))
    with pytest.raises(RuntimeError):
        dm.event_moments(torch.randn(4, 3))


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

    def moments(x=p, rowptr=p, B=3, N=10, F=4, max_len=0, mean=p, var=p):
        return lib.dmet_event_moments_f32(x, rowptr, B, N, F, max_len, mean, var, None)

    def dots(g=p, x=p, rowptr=p, B=3, N=10, F=4, max_len=0, shift=p, scale=p, s1=p, s2=p):
        return lib.dmet_event_dots_f32(g, x, rowptr, B, N, F, max_len, shift, scale, s1, s2, None)

    def affine(x=p, g=None, rowptr=p, B=3, N=10, F=4, shift=p, k1=p, k0=p, ka=None, out=p):
        return lib.dmet_event_affine_f32(x, g, rowptr, B, N, F, shift, k1, k0, ka, out, None)

    for call in (moments, dots, affine):
        for bad in (dict(F=0), dict(F=-1), dict(B=-1), dict(N=-1), dict(N=2 ** 31), dict(B=2 ** 31), dict(rowptr=None),
                    dict(x=None)):
            assert call(**bad) == -22, (call.__name__, bad)
            assert b"dmet_event_" in lib.dmet_last_error()
    for call in (moments, dots):
        assert call(max_len=-1) == -22
    assert moments(mean=None) == -22 and moments(var=None) == -22
    assert dots(g=None) == -22 and dots(s1=None) == -22 and dots(shift=None) == -22 and dots(scale=None) == -22
    assert dots(s2=None) == -22                                  # s2 goes with x, shift and scale
    assert affine(out=None) == -22 and affine(shift=None) == -22 and affine(k1=None) == -22 and affine(k0=None) == -22
    assert affine(g=p) == -22 and affine(ka=p) == -22            # g and ka together or not at all
    # empty problems are no-ops; what a request does not need may be NULL
    assert moments(B=0, x=None, mean=None, var=None) == 0 and dots(B=0) == 0 and affine(B=0) == 0 and affine(N=0, x=None) == 0
    assert dots(B=0, x=None, shift=None, scale=None, s2=None) == 0

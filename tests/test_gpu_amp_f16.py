"""PyTorch's standard mixed-precision recipe, torch.autocast("cuda") (float16) with torch.amp.GradScaler("cuda"), on
both models: the DynamicReductionNetwork (its EdgeConvs on the fp16 matrix-core route, csrc/edgemlp_bf16.hip) and the
drop-in StockNet with ops = deepmetv2_amd.  Accuracy against fp32 next to the bf16 recipes, the GradScaler contract
(a scaled tiny gradient keeps its bits; a scale past the fp16 range gives non-finite gradients, never saturated finite
ones, and the step is skipped), and end-to-end training."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F16 = "DMET_EDGE_MLP_F16"


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _count(monkeypatch, name):
    from deepmetv2_amd import _native
    calls = []
    real = getattr(_native, name)
    monkeypatch.setattr(_native, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _drn_data(dev, n_events, n_nodes, seed):
    g = torch.Generator().manual_seed(seed)
    data = type("D", (), {})()
    data.x = torch.randn(n_events * n_nodes, 5, generator=g).to(dev)
    data.batch = torch.repeat_interleave(torch.arange(n_events), n_nodes).to(dev)
    return data


def _pin_graphs(monkeypatch):
    """Record the kNN graphs and graclus clusters of the first DRN pass, replay them in every later pass (rewound by the
    returned callable), so that runs differ in precision only."""
    from deepmetv2_amd import drn
    rec = {"knn_graph": [], "graclus": []}
    pos = {"knn_graph": 0, "graclus": 0}
    replay = [False]

    def recorded(name, fn):
        def call(*a, **k):
            if replay[0]:
                pos[name] += 1
                return rec[name][pos[name] - 1]
            r = fn(*a, **k)
            rec[name].append(r)
            return r
        return call
    monkeypatch.setattr(drn, "knn_graph", recorded("knn_graph", drn.knn_graph))
    monkeypatch.setattr(drn, "graclus", recorded("graclus", drn.graclus))

    def rewind():
        replay[0] = True
        pos.update(knn_graph=0, graclus=0)
    return rewind


def _grads(m):
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None}


def _step(m, data, dtype=None, loss_scale=1.0, scaler=None, conv_dtype=None):
    """one forward + backward (no optimizer step): (output fp32, {param: grad}) -- grads unscaled when a scaler is given"""
    for conv in (m.edgeconv1, m.edgeconv2):
        conv.compute_dtype = conv_dtype
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=dtype or torch.float16, enabled=dtype is not None):
        out = m(data, seeds=(11, 12))
    loss = out.float().sum() * loss_scale
    if scaler is not None:
        scaler.scale(loss).backward()
    else:
        loss.backward()
    return out.detach().float(), _grads(m)


def _errors(out, grads, ref, ref_g):
    """(output error, largest gradient error): max |diff| over the fp32 output's max |.|, and per parameter max |diff|
    over that parameter's fp32 max |.|, the largest over the parameters"""
    assert grads.keys() == ref_g.keys()
    ge = max(_amax(grads[n] - ref_g[n]) / max(_amax(ref_g[n]), 1e-30) for n in ref_g)
    return _amax(out - ref) / max(_amax(ref), 1e-30), ge


def test_drn_fp16_autocast_is_closer_to_fp32_than_bf16(dev, monkeypatch):
    """4 x 1000, hidden 64, graphs and clusters pinned to the fp32 run's.  Under fp16 autocast both EdgeConvs take the
    fp16 route; its output and largest parameter-gradient error against fp32 are strictly below bf16 autocast's (the
    bf16 route).  With only the EdgeConvs under fp16 autocast (the rest of the model fp32), the fp16 route's output is
    no farther from fp32 than the generic route's (torch's fp16 recipe for the edge MLP, DMET_EDGE_MLP_F16=0).

    Measured on MI355X (output error / largest gradient error): full autocast, fp16 route 0.82 % / 7.0 %, bf16 route
    2.6 % / 45 %, generic route under fp16 autocast 0.68 % / 6.7 %.  Under full autocast the output error is torch's
    fp16 input and output Linears (the fp16 route alone moves the output by 0.057 %), and the two fp16 edge-MLP recipes
    land within that noise of each other on 4 outputs, so they are compared with the rest of the model in fp32:
    fp16 route 0.057 %, generic route 0.16 %."""
    import deepmetv2_amd as dm
    rewind = _pin_graphs(monkeypatch)
    f16 = _count(monkeypatch, "edge_mlp_fwd_f16")
    f16b = _count(monkeypatch, "edge_mlp_bwd_f16")
    bf16 = _count(monkeypatch, "edge_mlp_fwd_bf16")
    torch.manual_seed(35)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev)
    data = _drn_data(dev, 4, 1000, seed=36)
    ref, ref_g = _step(m, data)
    assert len(f16) == 0 and len(bf16) == 0
    res = {}
    for name, kw in (("f16", dict(dtype=torch.float16)), ("bf16", dict(dtype=torch.bfloat16)),
                     ("generic_f16", dict(dtype=torch.float16)), ("convs_f16", {}), ("convs_generic_f16", {})):
        rewind()
        if name.startswith("generic") or name == "convs_generic_f16":
            monkeypatch.setenv(F16, "0")
        if name.startswith("convs"):
            # only the two EdgeConvs under fp16 autocast, the rest of the model in fp32
            for conv in (m.edgeconv1, m.edgeconv2):
                conv.forward = _under_fp16_autocast(conv.forward)
        out, grads = _step(m, data, **kw)
        monkeypatch.delenv(F16, raising=False)
        for conv in (m.edgeconv1, m.edgeconv2):
            conv.__dict__.pop("forward", None)
        assert bool(torch.isfinite(out).all()), name
        for n, gr in grads.items():
            assert bool(torch.isfinite(gr).all()), (name, n)
        res[name] = _errors(out, grads, ref, ref_g)
    print("DRN vs fp32 (output, largest gradient error):", res)
    assert len(f16) == 4 and len(f16b) == 4 and len(bf16) == 2
    assert res["f16"][0] < res["bf16"][0] and res["f16"][1] < res["bf16"][1], res
    assert res["convs_f16"][0] <= res["convs_generic_f16"][0], res
    assert res["convs_f16"][0] <= 2e-3, res


def _under_fp16_autocast(fn):
    def call(*a, **k):
        with torch.autocast("cuda", dtype=torch.float16):
            return fn(*a, **k)
    return call


# ---- GradScaler contract --------------------------------------------------------------------------------------------------------
@pytest.fixture
def drn_2x1000(dev, monkeypatch):
    import deepmetv2_amd as dm
    rewind = _pin_graphs(monkeypatch)
    torch.manual_seed(47)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev)
    data = _drn_data(dev, 2, 1000, seed=48)
    ref, ref_g = _step(m, data)
    rewind()
    out, grads = _step(m, data, dtype=torch.float16)
    return m, data, rewind, (ref, ref_g), (out, grads), _errors(out, grads, ref, ref_g)


def test_gradscaler_keeps_scaled_tiny_gradients(dev, monkeypatch, drn_2x1000):
    """Loss times 2^-20 (tiny gradients).  With GradScaler(init_scale=2^20) the unscaled gradients match the fp32
    gradients of the same scaled-down loss as closely as the unscaled fp16 run matches fp32: the kernels round the
    scaled g_z2, not a flushed one.  Control: at scale 1 the same loss loses its gradients to fp16 underflow."""
    m, data, rewind, (ref, _ref_g), _f16, (_e_out, e_grad) = drn_2x1000
    calls = _count(monkeypatch, "edge_mlp_bwd_f16")
    tiny = 2.0 ** -20
    rewind()
    _o, ref_tiny = _step(m, data, loss_scale=tiny)
    errs = {}
    for scale in (2.0 ** 20, 1.0):
        rewind()
        scaler = torch.amp.GradScaler("cuda", init_scale=scale)
        out, _g = _step(m, data, dtype=torch.float16, loss_scale=tiny, scaler=scaler)
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        scaler.unscale_(opt)
        grads = _grads(m)
        for n, gr in grads.items():
            assert bool(torch.isfinite(gr).all()), (scale, n)
        errs[scale] = _errors(out, grads, ref, ref_tiny)[1]
    print("largest gradient error vs fp32 of the scaled-down loss:", errs, "unscaled fp16 run:", e_grad)
    assert len(calls) == 4
    assert errs[2.0 ** 20] <= 1.01 * e_grad + 1e-6, (errs, e_grad)
    assert errs[1.0] >= 10 * errs[2.0 ** 20] and errs[1.0] > 0.1, errs


def test_gradscaler_overflow_gives_non_finite_gradients_and_skips_the_step(dev, monkeypatch, drn_2x1000):
    """init_scale 2^40: every EdgeConv parameter gradient is non-finite or, after unscaling, matches the scale-1
    gradient within the fp16 run's accuracy; a finite wrong value (what saturation to 65504 gives) fails.  With any
    gradient non-finite the step leaves every parameter bit-identical and the scale drops."""
    m, data, rewind, (_ref, ref_g), (_out, g1), (_e_out, e_grad) = drn_2x1000
    rewind()
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    _step(m, data, dtype=torch.float16, scaler=scaler)
    scaler.unscale_(opt)
    grads = _grads(m)
    conv_names = [n for n in grads if n.startswith("edgeconv")]
    assert conv_names
    any_bad = False
    for n, gr in grads.items():
        if not bool(torch.isfinite(gr).all()):
            any_bad = True
            continue
        if n in conv_names:
            err = _amax(gr - g1[n]) / max(_amax(g1[n]), 1e-30)
            assert err <= max(e_grad, 1e-3), (n, err, e_grad)
    assert any_bad
    scaler.step(opt)
    scaler.update()
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    assert scaler.get_scale() < 2.0 ** 40


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _train(model_step, params, steps=20):
    opt = torch.optim.AdamW(params, lr=1e-3)
    scaler = torch.amp.GradScaler("cuda")
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda"):
            loss = model_step()
        assert loss.dtype == torch.float32
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
    return losses


def test_drn_trains_under_fp16_autocast_full_size(dev, monkeypatch):
    """64 x 4500, hidden 64, k 16: 20 AdamW steps under torch.autocast("cuda") + GradScaler on a fixed batch; both
    EdgeConvs on the fp16 route every step, the loss finite and lower at the end"""
    import deepmetv2_amd as dm
    calls = _count(monkeypatch, "edge_mlp_fwd_f16")
    torch.manual_seed(49)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev).train()
    data = _drn_data(dev, 64, 4500, seed=50)
    target = torch.randn(64, generator=torch.Generator().manual_seed(51)).to(dev)

    def step():
        out = m(data, seeds=(11, 12))
        return (out.float() - target).square().mean()
    losses = _train(step, m.parameters())
    print("DRN 64 x 4500 losses:", losses[0], losses[-1])
    assert len(calls) == 40
    assert all(map(lambda v: v == v and abs(v) != float("inf"), losses)), losses
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("variant", ["knn_graph", "dynamic", "static"])
def test_stock_net_trains_under_fp16_autocast(dev, variant):
    """The drop-in model with ops = deepmetv2_amd, the reference's loop under torch.autocast("cuda") + GradScaler:
    20 steps on a fixed batch, loss finite and lower at the end"""
    import deepmetv2_amd as dm
    from deepmetv2_amd import stock_model, synth
    sizes = [700, 90, 1300, 2500]
    x, y, batch, ptr = synth.make_events(sizes, seed=52, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes))
    torch.manual_seed(53)
    model = stock_model.StockNet(dm, 8, 3, variant=variant, k=16).to(dev).train()
    ei = None
    if variant == "static":
        etaphi = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1)
        ei = dm.radius_graph(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)

    def step():
        w = model(x[:, :8], x[:, 8:].long(), ei, batch)
        return stock_model.stock_loss_fn(dm, w, x, y, batch)
    losses = _train(step, model.parameters())
    print(variant, "losses:", losses[0], losses[-1])
    assert all(map(lambda v: v == v and abs(v) != float("inf"), losses)), losses
    assert losses[-1] < losses[0], losses

"""parallel.train_step / GraphedTrainStep on the models of tests/step_models.py: deeper than the library's queue of deferred
weight-gradient sums, with a layer applied twice, with frozen parameters, with BatchNorm in eval mode, at hidden 16 / 64.

1. one step against the float64 oracle over the same static graph;
2. three steps with the deferral on against three with it off, bit for bit, static and dynamic graph, and the number of
   sums the flush finds queued (step_models.expected_pending);
3. the memory a queued sum will write is still owned when the flush runs, also where autograd dropped the gradient;
4. shared and frozen steps under the poisoned allocations of tests/poisoned_alloc.py;
5. the captured step against the eager one."""
import os
import weakref

import pytest
import torch

import poisoned_alloc as pa
import step_models as sm

pytestmark = pytest.mark.gpu

# test_step_matches_float64_reference: 10 x the largest gradient error / gscale measured over the cases (see its docstring);
# never beyond the 2e-4 that test_full_model_train_step_matches_oracle grants
BAR = 4.6e-6
assert BAR <= 2e-4


def _fused_encoder() -> bool:
    return os.environ.get("DMET_FUSED_ENCODER", "1") != "0"


class _Rig:
    """Case `name` on the device with FlatModule (built after freezing), GradSync and an optimizer, and the batch."""

    def __init__(self, name, dev, flow="static", optimizer="flat", seed=sm.SEED):
        import deepmetv2_amd as dm
        from deepmetv2_amd.model import split_features
        from deepmetv2_amd.optim import FlatAdamW
        from deepmetv2_amd.parallel import FlatModule, GradSync
        self.name, self.dev, self.flow = name, dev, flow
        x, y, batch, ptr = sm.host_batch(seed)
        self.x, self.y, self.batch, self.ptr = x.to(dev), y.to(dev), batch.to(dev), ptr.to(dev)
        self.etaphi = sm.etaphi_of(x).to(dev)       # formed on the host, as the oracle's graph is: the same floats
        dm.register_batch(self.batch, self.ptr, len(sm.SIZES), max_nodes=max(sm.SIZES), min_nodes=min(sm.SIZES))
        self.model = sm.build_model(name, graph=flow)
        self.state0 = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        self.model.to(dev)
        if sm.CASES[name].bn_eval:
            sm.settle_bn_eval(self.model, lambda m: m(*split_features(self.x), self.graph(), self.batch))
        self.flat = FlatModule(self.model)
        self.sync = GradSync(self.flat)
        if optimizer == "flat":
            self.opt = FlatAdamW([self.flat.flat_param], lr=1e-3)
        else:
            self.opt = torch.optim.AdamW([self.flat.flat_param], lr=1e-3, capturable=True)
        self.names = [n for n, p in self.model.named_parameters() if p.requires_grad]
        self.frozen = [(n, p) for n, p in self.model.named_parameters() if not p.requires_grad]

    def graph(self, x=None):
        """The step's static graph as the counted radius table (train.py:45-48); None on the dynamic flow."""
        import deepmetv2_amd as dm
        if self.flow != "static":
            return None
        etaphi = self.etaphi if x is None else sm.etaphi_of(x)
        return dm.radius_table(etaphi, r=sm.RADIUS, batch=self.batch, loop=True, max_num_neighbors=255)

    def step(self, x=None, y=None):
        from deepmetv2_amd.parallel import train_step
        x = self.x if x is None else x
        return train_step(self.model, self.flat, self.sync, self.opt, x, self.y if y is None else y, self.batch,
                          self.ptr, edge_index=self.graph(x))


def test_device_graph_is_the_reference_graph(dev):
    """Both sides get the same edge set: the table the steps of test 1 convolve over holds exactly the oracle's edges
    (from the same host-made eta-phi floats; otherwise test 1 would compare two graphs)."""
    rig = _Rig("depth1", dev)
    el = rig.graph().edge_list()
    got = torch.stack([el.src.long(), el.tgt.long()]).cpu()
    ei = sm.host_graph()[5]

    def canon(e):
        return torch.unique(e[1] * (1 << 20) + e[0])       # (target, source) keys, sorted
    assert got.shape == ei.shape and torch.equal(canon(got), canon(ei))


# ---- 1. against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sm.CASES))
def test_step_matches_float64_reference(dev, name):
    """One train_step through FlatModule / GradSync / FlatAdamW, static graph, weight-gradient deferral on: the loss and
    every trainable parameter's gradient (flat.grad_views) against the float64 oracle, max|err| <= BAR * gscale with gscale
    the largest absolute reference gradient; then two more steps: frozen parameters keep their bits and get no .grad,
    eval-mode BatchNorm layers keep their running statistics.

    Measured on an MI355X, worst gradient error / gscale (and loss error / loss) per case:
        depth1 8.13e-08 (1.95e-08)   depth3 1.02e-07 (1.73e-08)   depth6 1.04e-07 (1.88e-08)   depth7 2.93e-07 (7.26e-08)
        depth9 1.84e-07 (1.03e-07)   shared2 1.90e-07 (1.05e-07)  shared3 2.41e-07 (2.62e-08)
        frozen_head 2.31e-07 (7.33e-08)   frozen_encoder, frozen_conv0, frozen_conv_bias, head_only 1.67e-07 (7.33e-08)
        bn_eval 2.53e-07 (2.94e-08)   hidden16 4.60e-07 (7.53e-08)   hidden64 3.06e-07 (8.13e-08)
    The kernels add in a fixed order: the figures repeat run to run.  BAR = 4.6e-6 is 10 x the largest of them (hidden16),
    far inside the 2e-4 of test_full_model_train_step_matches_oracle; the reference's own fp32 run is up to 9.3e-7 away
    from its float64 run (tests/test_step_models_host.py), and a single use of a shared weight 0.38 and more."""
    rig = _Rig(name, dev)
    loss_ref, grads_ref, gscale = sm.reference(name)      # from build_model's state: the state this rig started from
    assert all(torch.equal(v, rig.state0[k]) for k, v in sm.build_model(name).state_dict().items())
    assert [n for n, g in grads_ref.items() if g is not None] == rig.names
    frozen0 = [(n, p.detach().clone()) for n, p in rig.frozen]
    bns = sm.bn_layers(rig.model) if sm.CASES[name].bn_eval else []
    stats0 = [(bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()) for bn in bns]
    loss = rig.step()
    grads = [v.detach().cpu().double() for v in rig.flat.grad_views]
    worst, where = 0.0, None
    for n, g in zip(rig.names, grads):
        err = float((g - grads_ref[n]).abs().max()) / gscale
        if not err <= worst:        # (a NaN takes the lead and stays)
            worst, where = err, n
    loss_err = abs(float(loss) - float(loss_ref)) / abs(float(loss_ref))
    print(f"MEASURED {name}: worst gradient err / gscale = {worst:.3g} at {where}, gscale = {gscale:.4g}, "
          f"loss err / loss = {loss_err:.3g}")
    assert worst <= BAR, f"{name}: gradient of {where} is {worst:.3g} of the gradient scale from the float64 reference"
    assert loss_err <= BAR, f"{name}: loss {float(loss)!r} against {float(loss_ref)!r}"
    for _ in range(2):
        rig.step()
    for (n, p), (_n, p0) in zip(rig.frozen, frozen0):
        assert p.grad is None, f"{name}: frozen {n} got a gradient"
        assert pa.differing(p.detach(), p0).numel() == 0, f"{name}: frozen {n} changed"
    for bn, (m0, v0, t0) in zip(bns, stats0):
        assert torch.equal(bn.running_mean, m0) and torch.equal(bn.running_var, v0) and torch.equal(bn.num_batches_tracked, t0)


# ---- 2. deferred against not deferred --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", ["static", "dynamic"])
@pytest.mark.parametrize("name", list(sm.CASES))
def test_deferred_sums_same_bits_and_count(dev, monkeypatch, name, flow):
    """Three steps with _native.DEFER_FINALIZE on against three with it off: losses, flat_grad and flat_param carry the same
    bits, and every flush of the deferred run finds step_models.expected_pending sums queued (-1 without the deferral).
    The dynamic flow (k = 16) is held to these comparisons only."""
    from deepmetv2_amd import _lib, _native
    queued = []
    real_flush = _native.finalize_flush

    def counting_flush():
        queued.append(_lib.load().dmet_finalize_pending())
        real_flush()

    monkeypatch.setattr(_native, "finalize_flush", counting_flush)
    results = []
    for defer in (False, True):
        monkeypatch.setattr(_native, "DEFER_FINALIZE", defer)
        rig = _Rig(name, dev, flow=flow)
        n0 = len(queued)
        losses = [float(rig.step()) for _ in range(3)]
        assert len(queued) - n0 == 3
        results.append((losses, rig.flat.flat_grad.detach().clone(), rig.flat.flat_param.detach().clone(),
                        [b.detach().clone() for b in rig.model.buffers()]))
    (l0, g0, p0, b0), (l1, g1, p1, b1) = results
    assert l0 == l1, f"{name} {flow}: losses {l0} without the deferral, {l1} with it"
    assert pa.differing(g1, g0).numel() == 0, f"{name} {flow}: flat_grad differs in {pa.differing(g1, g0).numel()} elements"
    assert pa.differing(p1, p0).numel() == 0, f"{name} {flow}: flat_param differs"
    assert all(torch.equal(a, b) for a, b in zip(b0, b1))
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    n = sm.expected_pending(name, _fused_encoder())
    assert queued == [-1, -1, -1, n, n, n], f"{name} {flow}"
    assert _lib.load().dmet_finalize_pending() == -1


def test_head_and_encoder_applied_twice_inside_a_deferral(dev, monkeypatch):
    """The guard of a second use covers head_bwd and encode_bwd as well: two applications of one head, and of one encoder,
    inside one deferral give the gradients of the same backward pass without it, bit for bit, and leave nothing queued."""
    from deepmetv2_amd import _lib, _native, dense
    from per_node_reference import encoder_inputs, encoder_params
    g = torch.Generator().manual_seed(5)
    emb = [torch.randn(n, 32, generator=g).to(dev) for n in (700, 333)]
    x_cont, x_cat, _g = encoder_inputs(500, seed=6)
    x_cont, x_cat = x_cont.to(dev), x_cat.to(dev)
    monkeypatch.setattr(_native, "DEFER_FINALIZE", True)
    got = []
    for defer in (False, True):
        torch.manual_seed(2)
        lin1, lin2 = torch.nn.Linear(32, 16).to(dev), torch.nn.Linear(16, 1).to(dev)
        head = [lin1.weight, lin1.bias, lin2.weight, lin2.bias]
        enc = [p.to(dev).requires_grad_(True) for p in encoder_params(seed=11)]
        out = sum((dense.head(e, *head) * (i + 1.5)).sum() for i, e in enumerate(emb))
        h = dense.encode(x_cont, x_cat, *enc)
        out = out + (h * h).sum() + 0.5 * dense.encode(x_cont.flip(0), x_cat.flip(0), *enc).sum()
        if defer:
            assert _native.finalize_defer_begin()
        try:
            out.backward()
            if defer:
                assert _lib.load().dmet_finalize_pending() == 0
        finally:
            _native.finalize_flush()
        got.append([p.grad.clone() for p in head + enc])
    assert _lib.load().dmet_finalize_pending() == -1
    for a, b in zip(*got):
        assert bool(torch.isfinite(a).all()) and pa.differing(a, b).numel() == 0


# ---- 3. queued outputs outlive the queue -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["frozen_head", "frozen_encoder", "frozen_conv0", "head_only"])
def test_queued_outputs_outlive_the_queue(dev, monkeypatch, name):
    """Whatever edgeconv_linear_bwd, encode_bwd, encode_bn_bwd and head_bwd returned as a weight gradient inside a deferral
    is written by the flush through a raw pointer: at the flush, while sums are queued, the memory of every one of them
    must still be owned -- also where autograd dropped the gradient (a frozen parameter) during the pass.  Deterministic:
    it asks whether the storage is alive, not which block the allocator would hand out next.

    What is watched is each gradient's storage, not the tensor object: autograd takes a gradient over into .grad as a new
    tensor on the same storage, and only when nobody else holds the tensor (a second reference to it makes autograd COPY
    the still unwritten values), so the tensor object of a healthy step is gone by the flush while its memory is not."""
    from deepmetv2_amd import _lib, _native
    watched, checked = [], []

    def watch(fn_name, grads_of):
        real = getattr(_native, fn_name)

        def wrapper(*a, **kw):
            res = real(*a, **kw)
            if _native._DEFER["active"] and res is not None:
                for t in grads_of(res):
                    if t is not None:
                        watched.append((fn_name, tuple(t.shape), weakref.ref(t.untyped_storage())))
            return res
        monkeypatch.setattr(_native, fn_name, wrapper)

    watch("edgeconv_linear_bwd", lambda r: r[1:3])
    watch("encode_bwd", lambda r: r)
    watch("encode_bn_bwd", lambda r: r[0])
    watch("head_bwd", lambda r: r[1:])
    real_flush = _native.finalize_flush

    def checking_flush():
        pending = _lib.load().dmet_finalize_pending()
        if pending > 0:
            checked.append((pending, len(watched), [(f, s) for f, s, r in watched if r() is None]))
        watched.clear()
        real_flush()        # always: a deferral left open would spill into the next test

    monkeypatch.setattr(_native, "finalize_flush", checking_flush)
    monkeypatch.setattr(_native, "DEFER_FINALIZE", True)
    rig = _Rig(name, dev)
    for _ in range(2):
        rig.step()
    n = sm.expected_pending(name, _fused_encoder())
    assert [c[0] for c in checked] == ([n, n] if n > 0 else [])
    assert all(c[1] >= n for c in checked)
    for _pending, _n, dead in checked:
        assert not dead, f"{name}: the flush wrote {len(dead)} gradients whose memory had been released: {dead}"


# ---- 4. under poison -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shared2", "frozen_head"])
def test_step_under_poison(dev, name):
    """A step as allocated, under `ones` and under `zeros_huge`: the same bits, and each pattern did fill allocations.  An
    unwritten gradient that autograd adds to another (shared2), or a sum written into a block that meanwhile belongs to
    somebody else (frozen_head), shows as NaN / 3e38 here."""
    from test_gpu_poisoned_steps import _three_runs

    def make():
        rig = _Rig(name, dev)

        def step():
            loss = rig.step()
            return [("loss", loss), ("flat_grad", rig.flat.flat_grad), ("flat_param", rig.flat.flat_param)] + \
                   [(f"buffer {n}", b) for n, b in rig.model.named_buffers()]
        return step
    _three_runs(make, f"{name} step")


# ---- 5. captured -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth7", "shared2", "frozen_head"])
def test_captured_step_matches_eager(dev, name):
    """GraphedTrainStep with the static graph built inside the captured step (graph_fn -> radius_table), replayed three
    times with fresh inputs of the same shape: losses and flat_param equal the eager steps from the same state, bit for bit."""
    from deepmetv2_amd.parallel import GraphedTrainStep
    fresh = [sm.host_batch(seed)[:2] for seed in (31, 32, 33)]
    fresh = [(x.to(dev), y.to(dev)) for x, y in fresh]
    runs = []
    for graphed in (False, True):
        rig = _Rig(name, dev, optimizer="torch")
        if graphed:
            p0 = rig.flat.flat_param.detach().clone()
            bufs0 = [b.detach().clone() for b in rig.model.buffers()]
            xs, ys = rig.x.clone(), rig.y.clone()
            step = GraphedTrainStep(rig.model, rig.flat, rig.sync, rig.opt, xs, ys, rig.batch, rig.ptr, warmup=1,
                                    graph_fn=lambda xx: rig.graph(xx))
            with torch.no_grad():
                rig.flat.flat_param.copy_(p0)
                for b, b0 in zip(rig.model.buffers(), bufs0):
                    b.copy_(b0)
                for st in rig.opt.state.values():
                    for v in st.values():
                        if torch.is_tensor(v):
                            v.zero_()
        losses = []
        for x, y in fresh:
            if graphed:
                step.load(x, y)
                losses.append(float(step()))
            else:
                losses.append(float(rig.step(x, y)))
        torch.cuda.synchronize()
        runs.append((losses, rig.flat.flat_param.detach().clone()))
    assert len(set(runs[0][0])) == 3            # the inputs did change
    assert runs[0][0] == runs[1][0]
    assert pa.differing(runs[1][1], runs[0][1]).numel() == 0

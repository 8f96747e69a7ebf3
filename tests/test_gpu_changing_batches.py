"""Steps over CHANGING ragged batches, each against the same step run alone (tests/changing_batches.py).

The reference's loop (train.py:39-52) hands the model another ragged batch every step and validates between epochs; every
other whole-step test here feeds one batch again and again, which never makes stale what the package keeps between two
steps: the tensor-keyed registries, the prebuilt-graph slots of the EdgeConv layers, the kNN size hint, the
weight-gradient deferral, the memos of a NeighborTable, the kernel choice by event size.  Each test runs its sequence
once on one set of long-lived objects with a snapshot before every step, then runs every step alone -- new model,
FlatModule, GradSync and optimizer objects restored from the snapshot, new device tensors -- and asks for the same bits.
"""
import copy
import gc
import os

import pytest
import torch

import changing_batches as cb

pytestmark = pytest.mark.gpu


def _separate_bn(monkeypatch):
    """The BatchNorm transform as a launch of its own (the switches of test_gpu_poisoned_steps.test_net_train_step)."""
    from deepmetv2_amd import conv, dense
    monkeypatch.setattr(conv, "BN_KNN_FUSE", "0")
    monkeypatch.setattr(dense, "HEAD_FUSE", "0")
    monkeypatch.setenv("DMET_BN_NLS_FUSE", "0")


# ---- (a) Net(graph="dynamic") through parallel.train_step -----------------------------------------------------------------
@pytest.mark.parametrize("fuse", [True, False], ids=["fused-bn", "separate-bn"])
@pytest.mark.parametrize("optimizer", ["torch", "flat"])
def test_dynamic_hazards(dev, monkeypatch, optimizer, fuse):
    """Same N and B with another split, staging tensors refilled in place behind an inferred BatchInfo, tensors freed and
    allocated again, registered and inferred batches in turn, B and N up and down (empty, one-node and short-row events),
    the first batch again as the last; the learning rate changes twice (FlatAdamW.sync_hyper)."""
    if not fuse:
        _separate_bn(monkeypatch)
    make = cb.net_rig(dev, "dynamic", optimizer)
    records = cb.run_sequence(make(), cb.DYNAMIC_HAZARDS)
    assert sum(r[0].lr is not None for r in records) == 2
    assert all(bool(torch.isfinite(r[3][1][1])) for r in records)
    cb.check_alone(make, records, f"dynamic {optimizer} fuse={fuse}")


@pytest.mark.parametrize("fuse", [True, False], ids=["fused-bn", "separate-bn"])
def test_dynamic_kernel_thresholds(dev, monkeypatch, fuse):
    """max_nodes on each side of every size at which the code takes another kernel (16, 800, 1152, 2304, 4608, 5119), one
    batch after the other on the same objects."""
    if not fuse:
        _separate_bn(monkeypatch)
    make = cb.net_rig(dev, "dynamic", "flat")
    records = cb.run_sequence(make(), cb.DYNAMIC_THRESHOLDS)
    cb.check_alone(make, records, f"thresholds fuse={fuse}")


# ---- (b) Net(graph="static"): the step's radius graph handed over three ways ----------------------------------------------
@pytest.mark.parametrize("graph", ["table", "edge_index", "future"])
def test_static_hazards(dev, graph):
    make = cb.net_rig(dev, "static", "flat")
    records = cb.run_sequence(make(), cb.with_graph(cb.STATIC_HAZARDS, graph))
    cb.check_alone(make, records, f"static {graph}")


# ---- (c) what a real loop does between steps ------------------------------------------------------------------------------
class _Interrupt(Exception):
    pass


def test_steps_after_validation_and_interrupted_steps(dev, monkeypatch):
    """A validation pass, a step interrupted between forward and backward with the weight-gradient deferral begun, a forward
    interrupted between the encoder and the first convolution (its prebuilt kNN table is never consumed) and a forward the
    package refuses: the training step after each of them equals its run alone."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, conv, synth
    from deepmetv2_amd.model import loss_fn, split_features
    S = cb.Step
    make = cb.net_rig(dev, "dynamic", "flat")
    rig, stage, records = make(), {}, []
    conv0 = rig.model.graphnet.conv_continuous[0][0]

    def train(step, fuse=True):
        with monkeypatch.context() as m:
            if not fuse:
                m.setattr(conv, "BN_KNN_FUSE", "0")
            records.append((cb.run_sequence(rig, [step], stage)[0], fuse))
        assert not _native._DEFER["active"]
        dm.raise_deferred_errors()          # nothing that this step did not cause (and a sane step causes nothing)

    def forward_only(sizes, seed, registered):
        x, y, batch, ptr = synth.make_events(sizes, seed=seed, device=dev)
        if registered:
            dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
        rig.flat.zero_grad()
        w = rig.model(*split_features(x, lazy_cat=True), None, batch)
        return loss_fn(w, x, y, batch)

    train(S([300, 500], 601))
    # a validation pass on a batch of another size: no buffer moves
    before = [b.detach().clone() for b in rig.model.buffers()]
    xe, _ye, be, _pe = synth.make_events([700, 350], seed=602, device=dev)
    rig.model.eval()
    with torch.no_grad():
        w = rig.model(*split_features(xe), None, be)
    rig.model.train()
    assert w.shape == (1050,) and bool(torch.isfinite(w).all())
    for (name, b), b0 in zip(rig.model.named_buffers(), before):
        assert torch.equal(b, b0), f"{name} moved in an eval-mode forward"
    train(S([500, 300], 603))
    # a step interrupted between forward and backward, the deferral of its backward pass already begun
    with pytest.raises(_Interrupt):
        forward_only([450, 350], 604, False)
        _native.finalize_defer_begin()
        raise _Interrupt
    train(S([350, 450], 605, registered=False))
    # a forward interrupted before the first convolution takes the table that the encoder's BatchNorm had built for it; the
    # next step has the nodes of the interrupted one, another split, and builds its graphs itself
    def stop(*_a, **_k):
        raise _Interrupt
    with monkeypatch.context() as m:
        m.setattr(conv0, "forward_with_residual_input", stop)
        with pytest.raises(_Interrupt):
            forward_only([250, 550], 606, True)
    left = getattr(conv0, "_prebuilt", None) is not None
    if not any(name.startswith("DMET_") for name in os.environ):
        assert left, "the interrupted forward was expected to leave a prebuilt table behind"
    train(S([420, 380], 607, registered=False), fuse=False)
    assert getattr(conv0, "_prebuilt", None) is None
    # a forward the package refuses
    xu, _yu, bu, _pu = synth.make_events([300, 500], seed=608, device=dev)
    with pytest.raises(ValueError, match="sorted"):
        rig.model(*split_features(xu, lazy_cat=True), None, bu.flip(0).contiguous())
    train(S([300, 500], 601))
    for i, ((step, snap, host, out), fuse) in enumerate(records):
        with monkeypatch.context() as m:
            if not fuse:
                m.setattr(conv, "BN_KNN_FUSE", "0")
            cb.assert_same_bits(out, cb.run_alone(make, snap, host, step), i, f"between steps {step.sizes}")


# ---- (d) DynamicReductionNetwork: graclus registry, pair pooling, the 64-feature kNN ---------------------------------------
DRN_STEPS = [([120, 80], 701, "new"), ([80, 120], 702, "inplace"), ([1, 3, 0, 17, 129, 300], 703, "new"), ([200], 704, "new"),
             ([64, 0, 1, 90], 705, "new"), ([90, 1, 0, 64], 706, "inplace"), ([120, 80], 701, "new")]


def _drn_inputs(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(sizes), 5, generator=g)
    return x, torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _drn_step(m, data):
    m.zero_grad(set_to_none=True)
    out = m(data, seeds=(11, 12))
    loss = (out * out).sum()
    loss.backward()
    return ([("out", out.detach().clone()), ("loss", loss.detach().clone())]
            + [(f"grad {n}", (p.grad if p.grad is not None else torch.zeros_like(p)).clone()) for n, p in m.named_parameters()]
            + [(f"buffer {n}", b.detach().clone()) for n, b in m.named_buffers()])


def test_drn_sequence(dev):
    from deepmetv2_amd.drn import DynamicReductionNetwork

    def make():
        torch.manual_seed(2)
        return DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev).train()

    m, data, records = make(), type("D", (), {})(), []
    for sizes, seed, refill in DRN_STEPS:
        x, batch = _drn_inputs(sizes, seed)
        if refill == "inplace":
            data.x.copy_(x)
            data.batch.copy_(batch)
        else:
            data.x, data.batch = x.to(dev), batch.to(dev)
        snap = copy.deepcopy(m.state_dict())
        records.append((sizes, snap, (x, batch), _drn_step(m, data)))
    for i, (sizes, snap, (x, batch), out) in enumerate(records):
        alone, d = make(), type("D", (), {})()
        alone.load_state_dict(snap)
        d.x, d.batch = x.to(dev), batch.to(dev)
        assert out[0][1].shape == (len(sizes),)
        cb.assert_same_bits(out, _drn_step(alone, d), i, f"DRN {sizes}")


# ---- (e) GraphedTrainStep.load: fresh x, y of the captured shape ------------------------------------------------------------
def _graphed_batches(sizes):
    """x, y of the captured shape: ordinary events, a few rows repeated many times (exact ties far beyond k), extreme
    outliers, ordinary events again, the first batch again."""
    from deepmetv2_amd import synth
    out = []
    for seed, kind in ((801, "plain"), (802, "ties"), (803, "outliers"), (804, "plain"), (801, "plain")):
        x, y, _b, _p = synth.make_events(sizes, seed=seed)
        g = torch.Generator().manual_seed(seed)
        if kind == "ties":
            x = x[torch.randint(0, 5, (x.shape[0],), generator=g)].contiguous()          # 5 distinct rows in all
        elif kind == "outliers":
            rows = torch.randperm(x.shape[0], generator=g)[:40]
            x[rows, 2] = 500.0                                                            # pT at the generator's clamp
            x[rows[:20], 4] = 5000.0                                                      # d0, dz at theirs
            x[rows[20:], 5] = -5000.0
        out.append((kind, x, y))
    return out


def test_graphed_step_replays_fresh_batches(dev):
    """parallel.GraphedTrainStep fed through load(x, y) against the eager step on the same batches: loss and flat parameter
    bitwise after every step.  The kNN builds of a replay meet other ties and outliers than those of the capture."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, synth
    from deepmetv2_amd.model import Net
    from deepmetv2_amd.optim import FlatAdamW
    from deepmetv2_amd.parallel import FlatModule, GradSync, GraphedTrainStep, train_step
    sizes = [700, 90, 1300]
    x0, y0, batch, ptr = synth.make_events(sizes, seed=800, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    batches = _graphed_batches(sizes)
    runs, flagged = [], []
    for graphed in (False, True):
        torch.manual_seed(1)
        model = Net(8, 3, graph="dynamic", k=16).to(dev).train()
        flat = FlatModule(model); sync = GradSync(flat)
        opt = FlatAdamW([flat.flat_param], lr=1e-3)
        if graphed:
            p0 = flat.flat_param.detach().clone()
            bufs0 = [b.detach().clone() for b in model.buffers()]
            xs, ys = x0.clone(), y0.clone()
            step = GraphedTrainStep(model, flat, sync, opt, xs, ys, batch, ptr, warmup=1)
            with torch.no_grad():       # capture ran warm-up steps: rewind parameters, buffers and optimizer state
                flat.flat_param.copy_(p0)
                for b, b0 in zip(model.buffers(), bufs0):
                    b.copy_(b0)
                for st in opt.state.values():
                    for name, v in st.items():
                        if name == "bias_pow":
                            v.fill_(1.0)
                        elif torch.is_tensor(v) and name != "lr_dev":
                            v.zero_()
        trace = []
        for it, (kind, x, y) in enumerate(batches):
            if it == 3:
                opt.param_groups[0]["lr"] = 2.5e-4
            xd, yd = x.to(dev), y.to(dev)
            if graphed:
                step.load(xd, yd)
                loss = step()
            else:
                # which certification and fallback work the kNN build of this batch meets, on the eager embeddings
                with torch.no_grad():
                    probe = copy.deepcopy(model)
                    emb = probe.graphnet.embed(xd[:, :8], xd[:, 8:].long())
                    stats = {}
                    _native.knn_local(emb, ptr, 16, stats=stats)
                    print(f"graphed-load batch {it} ({kind}): kNN stats on the eager embeddings {stats}")
                    flagged.append(stats["flagged_queries"])
                loss = train_step(model, flat, sync, opt, xd, yd, batch, ptr)
            torch.cuda.synchronize()
            trace.append((float(loss), flat.flat_param.detach().clone()))
        runs.append(trace)
    for it, ((l0, p0), (l1, p1)) in enumerate(zip(*runs)):
        assert l0 == l1, f"step {it} ({batches[it][0]}): loss {l0!r} eager, {l1!r} replayed"
        cb.assert_same_bits([("flat_param", p0)], [("flat_param", p1)], it, f"graphed load ({batches[it][0]})")
    assert len({l for l, _ in runs[0][:-1]}) == len(batches) - 1
    if not any(name.startswith("DMET_") for name in os.environ):
        # on the default path the capture's batch flags no query and the tied one sends queries to the fallback: the replays
        # do meet other certification work than the capture (the outliers, as measured, flag none)
        assert flagged[0] == 0 and flagged[1] > 0, flagged


# ---- (f) the oracle on a changing sequence ------------------------------------------------------------------------------------
ORACLE_STEPS = [cb.Step([300, 40, 500], 901), cb.Step([500, 300, 40], 902), cb.Step([1, 700, 17], 903, registered=False),
                cb.Step([17, 1, 700], 904, registered=False, refill="inplace"), cb.Step([250, 9, 0, 400, 640], 905),
                cb.Step([1290], 906, registered=False)]


def test_changing_trajectory_matches_oracle(dev):
    """test_gpu_parity.test_training_trajectory_matches_oracle over six DIFFERENT batches: losses, final parameters and
    BatchNorm running statistics against oracle.ref_model.RefNet trained with stock torch.optim.AdamW on the CPU, with that
    test's bars (the +-lr-per-step bound of the zero-gradient biases taken over the six steps run here)."""
    from deepmetv2_amd.model import Net  # noqa: F401
    from oracle import ref_model, ref_ops
    steps = len(ORACLE_STEPS)
    rig = cb.net_rig(dev, "dynamic", "torch", seed=5)()
    ref = ref_model.RefNet(8, 3, graph="dynamic", k=16)
    ref.load_state_dict({n: v.detach().cpu().clone() for n, v in rig.model.state_dict().items()})
    ref.train()
    opt_ref = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    records = cb.run_sequence(rig, ORACLE_STEPS)
    losses = [float(r[3][1][1]) for r in records]
    losses_ref = []
    for _step, _snap, (x, y, batch, _ptr), _out in records:
        opt_ref.zero_grad()
        lr_ = ref_ops.loss_fn(ref(x[:, :8], x[:, 8:].long(), None, batch), x, y, batch)
        lr_.backward(); opt_ref.step()
        losses_ref.append(float(lr_.detach()))
    for a, b in zip(losses, losses_ref):
        assert abs(a - b) <= 2e-4 * abs(b) + 1e-3, (losses, losses_ref)
    sd, sd_ref = rig.model.state_dict(), ref.state_dict()
    for name in sd_ref:
        a, b = sd[name].detach().cpu(), sd_ref[name]
        if not a.is_floating_point():
            assert torch.equal(a, b), name
        elif name.endswith("nn.0.bias") or name.endswith("encode_all.0.bias"):
            assert float((a - b).abs().max()) <= 2 * steps * 1e-3 * 1.05, name   # each side moves at most lr per step
        elif name.endswith("running_mean"):
            torch.testing.assert_close(a, b, rtol=2e-3, atol=2 * steps * 1e-3 * 1.05, msg=lambda m, n=name: f"{n}: {m}")
        else:
            torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-4, msg=lambda m, n=name: f"{n}: {m}")


# ---- (g) nothing accumulates ---------------------------------------------------------------------------------------------------
def test_repeated_step_allocates_nothing_more(dev):
    """One step eight times on the same objects with new input tensors each time: the device memory in use after repetitions
    3..8 is one value."""
    from deepmetv2_amd import synth
    step = cb.Step([300, 40, 500], 1001)
    rig = cb.net_rig(dev, "dynamic", "flat")()
    host = synth.make_events(step.sizes, seed=step.seed)
    used = []
    for _ in range(8):
        t = cb.present(step, host, dev)
        out = cb.one_step(rig, t, step)
        del t, out
        rig.seen.clear()
        gc.collect()        # the figure is the process's: garbage of whatever ran before must not be freed between two readings
        torch.cuda.synchronize()
        used.append(torch.cuda.memory_allocated(dev))
    assert len(set(used[2:])) == 1, used


def test_registries_do_not_grow_with_the_steps(dev):
    """After a run of the static flow over radius_graph's [2,E] tensors and of the DRN (to_undirected, graclus) and
    gc.collect(), no registry holds an entry of a dead tensor, and their lengths are those after half as many steps."""
    from deepmetv2_amd.drn import DynamicReductionNetwork
    torch.manual_seed(2)
    drn = DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev).train()
    rig, stage, data = cb.net_rig(dev, "static", "flat")(), {}, type("D", (), {})()
    steps = cb.with_graph(cb.STATIC_HAZARDS[:5] + cb.STATIC_HAZARDS[7:] + cb.STATIC_HAZARDS[:2], "edge_index")
    assert len(steps) == 9
    lengths = []
    for lo, hi in ((0, 4), (4, 8)):
        cb.run_sequence(rig, steps[lo:hi], stage)
        for sizes, seed, _r in DRN_STEPS[lo:hi]:
            x, batch = _drn_inputs(sizes, seed)
            data.x, data.batch = x.to(dev), batch.to(dev)
            _drn_step(drn, data)
        stage.clear()
        data.x = data.batch = None
        rig.seen.clear()
        gc.collect()
        regs = cb.registries()
        assert {name: cb.dead_entries(r) for name, r in regs.items()} == {name: [] for name in regs}
        lengths.append({name: len(r) for name, r in regs.items()})
    assert lengths[0] == lengths[1], lengths

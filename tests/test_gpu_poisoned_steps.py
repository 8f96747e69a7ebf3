"""Whole steps with every allocation of deepmetv2_amd/_native.py filled beforehand (tests/poisoned_alloc.py), NO masks.

tests/test_gpu_poisoned_buffers.py lets a producer leave the regions include/dmet.h declares unwritten; that is only safe
if no consumer reads behind them.  Here one forward, loss and backward of each model runs three times -- as allocated,
under `ones` and under `zeros_huge` -- on a ragged batch with a one-node, a three-node, an empty and a 900-node event (the
matrix-core kNN path is in the step), graph builds included.  Every output, the loss, every parameter gradient and
every buffer must have the same bits in the three runs."""
import copy

import pytest
import torch

import poisoned_alloc as pa

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 0, 17, 129, 900]


def _three_runs(make, what):
    """make() -> a fresh step() -> list of (name, tensor); bitwise equality of the three runs."""
    plain = [(n, t.detach().cpu()) for n, t in make()()]
    assert plain, what
    for pattern in pa.PATTERNS:
        step = make()                       # models, inputs and optimizer state: built outside the block
        with pa.poisoned(pattern) as p:
            got = step()
        torch.cuda.synchronize()
        assert p.count > 0, f"{what}: nothing was poisoned under {pattern}"
        assert [n for n, _ in got] == [n for n, _ in plain], what
        for (name, a), (_n, b) in zip(got, plain):
            bad = pa.differing(a.detach().cpu(), b)
            assert bad.numel() == 0, (f"{what}: {name} {tuple(b.shape)} differs under {pattern} from the unpoisoned run in "
                                      f"{bad.numel()} elements, first at flat index {int(bad[0])}")


def _named_grads(module):
    return [(f"grad {n}", p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in module.named_parameters()] + \
           [(f"buffer {n}", b) for n, b in module.named_buffers()]


# ---- (a) model.Net through parallel.train_step, weight-gradient deferral on ------------------------------------------------
@pytest.mark.parametrize("flow", ["dynamic", "static-table"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fused-bn", "separate-bn"])
def test_net_train_step(dev, monkeypatch, flow, fuse):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, conv, dense, synth
    from deepmetv2_amd.model import Net
    from deepmetv2_amd.parallel import FlatModule, GradSync, train_step
    if not fuse:        # the BatchNorm transform as a launch of its own: not inside the next build, not inside the head
        monkeypatch.setattr(conv, "BN_KNN_FUSE", "0")
        monkeypatch.setattr(dense, "HEAD_FUSE", "0")
        monkeypatch.setenv("DMET_BN_NLS_FUSE", "0")
    x, y, batch0, ptr0 = synth.make_events(SIZES, seed=5, device=dev)

    def make():
        # a batch vector of its own per run: whatever the registry caches for a batch is rebuilt, on this run's buffers
        batch, ptr = batch0.clone(), ptr0.clone()
        dm.register_batch(batch, ptr, len(SIZES), max_nodes=max(SIZES))
        torch.manual_seed(1)
        model = Net(8, 3, graph="dynamic" if flow == "dynamic" else "static", k=16).to(dev).train()
        flat = FlatModule(model)
        sync = GradSync(flat)
        opt = torch.optim.AdamW([flat.flat_param], lr=1e-3)
        seen = []
        model.register_forward_hook(lambda _m, _i, out: seen.append(out.detach().clone()))

        def step():
            graph = None
            if flow == "static-table":      # rows with counts (pad=False inside): the reference's active flow, train.py:45-48
                etaphi = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1)
                graph = dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)
                assert graph.cnt is not None
            loss = train_step(model, flat, sync, opt, x, y, batch, ptr, edge_index=graph)
            assert not _native._DEFER["active"]
            return [("weights", seen[-1]), ("loss", loss), ("flat_grad", flat.flat_grad), ("flat_param", flat.flat_param)] + \
                   [(f"buffer {n}", b) for n, b in model.named_buffers()]
        return step
    _three_runs(make, f"Net {flow} fuse={fuse}")


# ---- (b) DynamicReductionNetwork: coarsening, pair pooling, the 64-feature kNN ----------------------------------------------
def test_drn_step(dev):
    from deepmetv2_amd.drn import DynamicReductionNetwork
    g = torch.Generator().manual_seed(3)
    data = type("D", (), {})()
    data.x = torch.randn(sum(SIZES), 5, generator=g).to(dev)
    data.batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES)).to(dev)

    def make():
        torch.manual_seed(2)
        m = DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev).train()

        def step():
            out = m(data, seeds=(11, 12))
            loss = (out * out).sum()
            loss.backward()
            return [("out", out), ("loss", loss)] + _named_grads(m)
        return step
    _three_runs(make, "DRN")


# ---- (c) GravNetConv and TransformerConv, one layer each, one set and two -----------------------------------------------------
@pytest.mark.parametrize("kind", ["gravnet", "gravnet-xy", "transformer-table", "transformer-list", "transformer-xy"])
def test_aggregation_layers(dev, kind):
    import deepmetv2_amd as dm
    import attention_reference as ar
    from test_gpu_gravnet import _ragged
    batch, N = _ragged(SIZES, dev)
    sy = [2, 0, 5, 9, 64, 130]                       # queries of the two-set forms: an event with queries and no candidate
    by, Ny = _ragged(sy, dev)
    g = torch.Generator().manual_seed(31)
    x, xq = torch.randn(N, 12, generator=g).to(dev), torch.randn(Ny, 12, generator=g).to(dev)
    coords = ar.coords(N, 32).to(dev)
    ei = torch.stack([torch.randint(0, N, (4000,), generator=g), torch.randint(0, Ny - 3, (4000,), generator=g)]).to(dev)

    def make():
        torch.manual_seed(30)
        if kind.startswith("gravnet"):
            conv = dm.GravNetConv(12, 14, 4, 22, 16).to(dev)
        else:
            conv = dm.TransformerConv((12, 12) if kind == "transformer-xy" else 12, 16, heads=4, beta=True).to(dev)

        def step():
            xx, xr = x.clone().requires_grad_(True), xq.clone().requires_grad_(True)
            if kind == "gravnet":
                out = conv(xx, batch)
            elif kind == "gravnet-xy":
                out = conv((xx, xr), (batch, by))
            elif kind == "transformer-table":
                out = conv(xx, dm.knn_table(coords, 16, batch, loop=True))
            elif kind == "transformer-list":
                nbr = dm.knn_table(coords, 16, batch, loop=True).nbr        # the same graph as a plain [2, E] tensor
                i, t = (nbr >= 0).nonzero(as_tuple=True)
                out = conv(xx, torch.stack([nbr[i, t].long(), i]))
            else:
                out = conv((xx, xr), ei)
            loss = (out * out).sum()
            loss.backward()
            gr_ = [("gx", xx.grad)] + ([("gx_r", xr.grad)] if xr.grad is not None else [])
            return [("out", out), ("loss", loss)] + gr_ + _named_grads(conv)
        return step
    _three_runs(make, kind)


# ---- (d) EdgeConv with an MLP message: fp32, bf16 autocast, fp16 autocast + GradScaler -----------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16-scaler"])
@pytest.mark.parametrize("aggr", ["max", "add"])
def test_edgeconv_mlp_step(dev, mode, aggr):
    import deepmetv2_amd as dm
    from test_gpu_edge_mlp_f32 import _knn_sym, _mlp
    xd, _bd, ei = _knn_sym(dev, SIZES, 6, 32, seed=4)
    nn0 = _mlp(32, 48, 32, bn="train", seed=7)
    dtype = {"fp32": None, "bf16": torch.bfloat16, "fp16-scaler": torch.float16}[mode]

    def make():
        conv = dm.EdgeConv(copy.deepcopy(nn0), aggr=aggr)
        conv.nn.load_state_dict(nn0.state_dict())
        conv = conv.to(dev).train()
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0) if mode == "fp16-scaler" else None

        def step():
            xx = xd.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=dtype or torch.float16, enabled=dtype is not None):
                out = conv(xx, ei)
            loss = (out.float() ** 2).sum()
            (scaler.scale(loss) if scaler is not None else loss).backward()
            return [("out", out.float()), ("loss", loss), ("gx", xx.grad)] + _named_grads(conv)
        return step
    _three_runs(make, f"EdgeConv {mode} {aggr}")

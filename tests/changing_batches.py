"""TEST INFRASTRUCTURE for tests/test_gpu_changing_batches.py and tests/test_changing_batches_host.py: steps over CHANGING
ragged batches on one set of long-lived objects, each compared bit for bit with the same step run alone.

Between two steps the package keeps state that one repeated batch never makes stale: the tensor-keyed registries of
graph.py / pool.py, the prebuilt-graph slots of the EdgeConv layers, the kNN size hint, the weight-gradient deferral, the
memos of a NeighborTable, and which kernel a batch's event sizes select.  A run ALONE starts from none of it: new model,
FlatModule, GradSync and optimizer objects with the state of a snapshot taken right before the step, and new device
tensors made from host copies of the batch, presented the way the sequence presented them.

The sequences are data (`Step` tuples): every pair of consecutive batches is there for one hazard, named in its comment.
"""
from __future__ import annotations

import copy
from collections import namedtuple

import torch

# sizes, seed: synth.make_events(sizes, seed).  registered: register_batch(ptr, B, max_nodes, min_nodes) as DeviceLoader
# does, else the operators infer (and remember) the events from the vector.  graph: None (the model builds its kNN graphs)
# or how the step's radius graph is handed over: "table" / "edge_index" / "future".  refill: "new" tensors, the previous
# step's x / y / batch objects filled "inplace" (copy_, with a new ptr), or "realloc" (the previous ones deleted first and
# the same sizes allocated again: the allocator may hand back the same addresses, CPython the same ids).  lr: the
# learning rate a scheduler sets before this step (None: unchanged).
Step = namedtuple("Step", "sizes seed registered graph refill lr", defaults=(True, None, "new", None))

K = 16

# ---- (a) dynamic flow: the hazards of a changing run -------------------------------------------------------------------
DYNAMIC_HAZARDS = [
    Step([300, 500], 101),                                   # the first batch (it comes again as the last)
    Step([500, 300], 102),                                   # same N and B, different split: every tensor shape is equal
    Step([330, 470], 103, registered=False),                 # not registered: its BatchInfo is inferred and remembered
    Step([470, 330], 104, registered=False, refill="inplace", lr=4e-4),   # same objects refilled, new ptr, other split
    Step([420, 380], 105, refill="realloc"),                 # freed and allocated again, registered behind an inferred entry
    Step([390, 410], 106, registered=False, refill="realloc"),            # ... and inferred behind a registered one
    Step([40, 0, 1, 7, 900, 15, 16], 107, lr=2.5e-3),        # B and N up: empty, one node, rows shorter than k, k itself, > 800
    Step([120], 108, registered=False),                      # B and N down to one small event
    Step([0, 5, 0, 33, 2], 109, registered=False),           # leading and inner empty events, every event shorter than 2 k
    Step([300, 500], 101),                                   # the first batch again
]

# max_nodes on each side of every size at which the code switches kernels: k = 16, the kNN filter's forms (800), the windows
# of gather_max_bwd_lds_kernel (1152, 2304, 4608), conv._LDS_MAX_EVENT_NODES (5119); registered and inferred in turn
DYNAMIC_THRESHOLDS = [
    Step([16, 16, 9], 201),
    Step([17, 3], 202, registered=False),
    Step([800, 420], 203),
    Step([801, 800], 204, registered=False),                 # min_nodes = 800: the size hint says "second form only"
    Step([1152, 30], 205),
    Step([1153, 1152], 206, registered=False),
    Step([2304, 100], 207),
    Step([2305], 208, registered=False),
    Step([4608, 850], 209),
    Step([4609, 40], 210, registered=False),
    Step([5119, 1, 0, 900], 211),
    Step([5120, 5119], 212, registered=False),
]

# ---- (b) static flow: one radius graph per step ------------------------------------------------------------------------
STATIC_HAZARDS = [
    Step([300, 500], 301),
    Step([500, 300], 302),                                   # same N and B, different split
    Step([330, 470], 303, registered=False),
    Step([470, 330], 304, registered=False, refill="inplace", lr=4e-4),
    Step([420, 380], 305, refill="realloc"),
    Step([5119, 300, 0, 1], 306, lr=2.5e-3),                 # the LDS image's largest event, an empty and a one-node event
    Step([5120, 200], 307, registered=False),                # one node beyond it: row-major P / Q
    Step([60, 7], 308, registered=False),
    Step([300, 500], 301),
]

# ---- the same hazards at sizes the CPU stand-in walks in a second ------------------------------------------------------------
HOST_DYNAMIC = [
    Step([30, 40], 401),
    Step([40, 30], 402),
    Step([33, 37], 403, registered=False),
    Step([45, 25], 404, registered=False, refill="inplace", lr=4e-4),     # the step a stale inferred BatchInfo would break
    Step([42, 28], 405, refill="realloc"),
    Step([39, 31], 406, registered=False, refill="realloc"),
    Step([20, 0, 1, 7, 50, 15, 16, 17], 407, lr=2.5e-3),
    Step([24], 408, registered=False),
    Step([0, 5, 0, 33, 2], 409, registered=False),
    Step([30, 40], 401),
]
HOST_STATIC = [
    Step([30, 40], 501),
    Step([40, 30], 502),
    Step([33, 37], 503, registered=False),
    Step([45, 25], 504, registered=False, refill="inplace", lr=4e-4),
    Step([42, 28], 505, refill="realloc"),
    Step([90, 0, 1, 12], 506, lr=2.5e-3),
    Step([24], 507, registered=False),
    Step([30, 40], 501),
]


def with_graph(steps, graph):
    return [s._replace(graph=graph) for s in steps]


# ---- the objects of a run ------------------------------------------------------------------------------------------------
class Rig:
    """model, FlatModule, GradSync, optimizer; `seen` collects the model's outputs (a forward hook)."""

    def __init__(self, model, optimizer_of):
        from deepmetv2_amd.parallel import FlatModule, GradSync
        self.model = model
        self.flat = FlatModule(model)
        self.sync = GradSync(self.flat)
        self.opt = optimizer_of(self.flat.flat_param)
        self.seen = []
        model.register_forward_hook(lambda _m, _i, out: self.seen.append(out.detach().clone()))

    @property
    def device(self):
        return self.flat.flat_param.device


def net_rig(dev, graph, optimizer="torch", seed=1):
    """make() for Net(graph=..., k=16) in training mode; optimizer: "torch" (torch.optim.AdamW) or "flat" (optim.FlatAdamW)."""
    def make():
        from deepmetv2_amd.model import Net
        torch.manual_seed(seed)
        model = Net(8, 3, graph=graph, k=K).to(dev).train()
        if optimizer == "flat":
            from deepmetv2_amd.optim import FlatAdamW
            return Rig(model, lambda p: FlatAdamW([p], lr=1e-3))
        return Rig(model, lambda p: torch.optim.AdamW([p], lr=1e-3))
    return make


# ---- snapshot / restore --------------------------------------------------------------------------------------------------
def snapshot(model, flat, opt):
    """The flat parameter, every buffer and the optimizer's state_dict, all as copies."""
    return {"flat_param": flat.flat_param.detach().clone(),
            "buffers": [b.detach().clone() for b in model.buffers()],
            "opt": copy.deepcopy(opt.state_dict())}


def restore(snap, model, flat, opt):
    """snapshot's inverse, onto freshly constructed objects.  The optimizer takes the snapshot's learning rate as one it was
    given (FlatAdamW's device copy of it is not restored but formed anew), and state that load_state_dict would cast to the
    parameter's dtype (FlatAdamW's float64 bias_pow) is put back as it was."""
    with torch.no_grad():
        flat.flat_param.copy_(snap["flat_param"])
        for b, b0 in zip(model.buffers(), snap["buffers"]):
            b.copy_(b0)
    sd = copy.deepcopy(snap["opt"])
    for st in sd["state"].values():
        st.pop("lr_dev", None)
        st.pop("lr_host", None)
    opt.load_state_dict(sd)
    params = [p for g in opt.param_groups for p in g["params"]]
    for idx, st in sd["state"].items():
        for name, v in st.items():
            if torch.is_tensor(v) and opt.state[params[idx]][name].dtype != v.dtype:
                opt.state[params[idx]][name] = v.clone().to(opt.state[params[idx]][name].device)


# ---- presenting a batch --------------------------------------------------------------------------------------------------
def host_batch(step):
    from deepmetv2_amd import synth
    return synth.make_events(step.sizes, seed=step.seed)


def present(step, host, dev, stage=None):
    """The batch of `host` = (x, y, batch, ptr) as device tensors, allocated as step.refill says (`stage`: the tensors of the
    sequence's previous step; None = a run alone, always new tensors) and registered or not.  Returns the dict of tensors."""
    import deepmetv2_amd as dm
    names = ("x", "y", "batch", "ptr")
    refill = step.refill if stage else "new"
    if stage is None:
        stage = {}
    if refill == "inplace":
        for n, h in zip(names[:3], host[:3]):
            assert stage[n].shape == h.shape, "an in-place refill needs the previous step's N and B"
            stage[n].copy_(h)
        stage["ptr"] = host[3].clone().to(dev)
    else:
        if refill == "realloc":
            assert all(stage[n].shape == h.shape for n, h in zip(names, host)), "realloc: the previous step's N and B"
            stage.clear()                                   # freed first: the allocator may hand the same blocks back
        for n, h in zip(names, host):
            stage[n] = h.clone().to(dev)
    if step.registered:
        dm.register_batch(stage["batch"], stage["ptr"], len(step.sizes), max_nodes=max(step.sizes), min_nodes=min(step.sizes))
    return stage


def build_graph(kind, x, batch):
    """The step's radius graph (train.py:45-48) as the counted table, radius_graph's [2,E] tensor or a side-stream future."""
    import deepmetv2_amd as dm
    if kind is None:
        return None
    etaphi = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1)
    if kind == "edge_index":
        return dm.radius_graph(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)
    build = lambda: dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255)     # noqa: E731
    return dm.build_async(build) if kind == "future" else build()


def one_step(rig, t, step):
    """parallel.train_step on the tensors `t`; the named tensors a step is compared by, as copies."""
    from deepmetv2_amd.parallel import train_step
    graph = build_graph(step.graph, t["x"], t["batch"])
    loss = train_step(rig.model, rig.flat, rig.sync, rig.opt, t["x"], t["y"], t["batch"], t["ptr"], edge_index=graph)
    del graph
    return ([("weights", rig.seen[-1]), ("loss", loss.clone()), ("flat_grad", rig.flat.flat_grad.detach().clone()),
             ("flat_param", rig.flat.flat_param.detach().clone())]
            + [(f"buffer {n}", b.detach().clone()) for n, b in rig.model.named_buffers()])


def run_sequence(rig, steps, stage=None):
    """Every step on the long-lived objects of `rig`; -> [(step, snapshot before it, host batch, outputs)]."""
    stage = {} if stage is None else stage
    records = []
    for step in steps:
        if step.lr is not None:
            rig.opt.param_groups[0]["lr"] = step.lr            # a scheduler steps between two training steps
        host = host_batch(step)
        t = present(step, host, rig.device, stage)
        snap = snapshot(rig.model, rig.flat, rig.opt)
        records.append((step, snap, host, one_step(rig, t, step)))
    return records


def run_alone(make, snap, batch_on_host, how):
    """One step on new objects (make()) holding the state of `snap`, on new device tensors made from `batch_on_host`,
    presented as the Step `how` says."""
    rig = make()
    restore(snap, rig.model, rig.flat, rig.opt)
    return one_step(rig, present(how, batch_on_host, rig.device), how)


def assert_same_bits(seq_outputs, alone_outputs, step, what):
    assert [n for n, _ in seq_outputs] == [n for n, _ in alone_outputs], f"{what}, step {step}: different outputs"
    for (name, a), (_n, b) in zip(seq_outputs, alone_outputs):
        a, b = a.detach().cpu(), b.detach().cpu()
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}, step {step}: {name} is {a.dtype}{tuple(a.shape)} in the " \
                                                          f"sequence, {b.dtype}{tuple(b.shape)} alone"
        if not torch.equal(a, b):
            bad = torch.nonzero(a.reshape(-1) != b.reshape(-1)).view(-1)
            first = int(bad[0]) if bad.numel() else -1      # (-1: equal values that are not equal to themselves, NaN)
            va = a.reshape(-1)[first].item() if bad.numel() else float("nan")
            vb = b.reshape(-1)[first].item() if bad.numel() else float("nan")
            raise AssertionError(f"{what}, step {step}: {name} {tuple(a.shape)} differs from the step run alone in "
                                 f"{bad.numel()} elements, first at flat index {first} ({va!r} in the sequence, {vb!r} alone)")


def check_alone(make, records, what):
    for i, (step, snap, host, out) in enumerate(records):
        assert_same_bits(out, run_alone(make, snap, host, step), i, f"{what} {step.sizes}")


def dead_entries(reg):
    """Keys of a tensor-keyed registry whose weakref is dead."""
    return [key for key, ent in reg.items() if ent[0]() is None]


def registries():
    from deepmetv2_amd import graph, pool
    return {"batch": graph._batch_registry, "graph": graph._graph_registry, "coalesced": graph._coalesced_registry,
            "graclus": pool._graclus_registry}

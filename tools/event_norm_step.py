"""Forward + backward time of GraphNorm and LayerNorm(mode='graph') (csrc/event_norm.hip) against the same formulas
composed from this package's scatter_mean plus torch indexing, and against this package's nn.BatchNorm1d for scale.

    python tools/event_norm_step.py [--steps 50] [--warmup 10] [--json OUT]

Two batches of the same total, F = 64 fp32: 64 events of 4500 nodes, and 64 events of 500 to 8000 nodes (seeded,
adjusted to the same 288 000).  One JSON line per batch.  The variants take turns inside one loop; medians of
the per-step device time (HIP events), gradients to x and to every parameter.  `floor_us`: the traffic floor of the
fused route at the measured copy rate of 6.29 TB/s -- forward 2 N F 4 bytes (read x, write y; the second walk of the
variance comes from L2), backward 3 N F 4 bytes (read g and x, write g_x; the second read of both comes from L2) -- and
`floor_fraction` = floor / fused time.  `kernels`: HIP-event brackets of the three native calls in a run of their own.
`max_abs_diff`: fused against composed outputs at the timed size."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native  # noqa: E402
from deepmetv2_amd.nn import BatchNorm1d  # noqa: E402

F, B, TOTAL = 64, 64, 64 * 4500
COPY_RATE = 6.29e12        # bytes / s, the measured float4 copy rate of the MI355X


def composed_graph_norm(mod, x, batch, nb):
    mean = dm.scatter_mean(x, batch, dim=0, dim_size=nb)
    out = x - mean.index_select(0, batch) * mod.mean_scale
    var = dm.scatter_mean(out * out, batch, dim=0, dim_size=nb)
    std = (var + mod.eps).sqrt().index_select(0, batch)
    return mod.weight * out / std + mod.bias


def composed_layer_norm(mod, x, batch, nb):
    mean = dm.scatter_mean(x, batch, dim=0, dim_size=nb).mean(-1, keepdim=True)
    out = x - mean.index_select(0, batch)
    var = dm.scatter_mean(out * out, batch, dim=0, dim_size=nb).mean(-1, keepdim=True)
    out = out / (var + mod.eps).sqrt().index_select(0, batch)
    return out * mod.weight + mod.bias


def ragged_lengths(seed=0):
    """B lengths drawn uniformly from [500, 8000], then moved towards the total in turns of at most 256 nodes."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(500, 8001, (B,), generator=g).tolist()
    diff = TOTAL - sum(n)
    while diff:
        for i in range(B):
            d = min(diff, 8000 - n[i], 256) if diff > 0 else -min(-diff, n[i] - 500, 256)
            n[i] += d
            diff -= d
    return n


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def alternate(fns, steps, warmup, dev):
    """{name: [ms]}: the variants take turns inside one loop, so drift of the machine reaches all of them alike."""
    ev = {name: [] for name in fns}
    for it in range(warmup + steps):
        for name, fn in fns.items():
            pair = timed(fn)
            if it >= warmup:
                ev[name].append(pair)
    torch.cuda.synchronize(dev)
    return {name: [a.elapsed_time(b) for a, b in pairs] for name, pairs in ev.items()}


def bracket(names, fn, steps, dev):
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, set(names)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    out = {name: round(ms * 1e3, 2) for name, (_count, ms) in _native.timer.summary().items()}
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()
    return out


def run_batch(label, lengths, steps, warmup, dev):
    g = torch.Generator().manual_seed(1)
    N = sum(lengths)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(lengths).cumsum(0)]).to(dev)
    batch = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths)).to(dev)
    dm.register_batch(batch, ptr, len(lengths), max_nodes=max(lengths), min_nodes=min(lengths))
    x = torch.randn(N, F, generator=g).to(dev)
    gout = torch.randn(N, F, generator=g).to(dev)
    xx = x.clone().requires_grad_(True)
    torch.manual_seed(2)
    gn, ln, bn = dm.GraphNorm(F).to(dev), dm.LayerNorm(F).to(dev), BatchNorm1d(F).to(dev)
    with torch.no_grad():
        for m in (gn, ln):
            for p in m.parameters():
                p.add_(0.1 * torch.randn_like(p))
    nb = len(lengths)

    def step(fn, mod):
        leaves = (xx,) + tuple(mod.parameters())

        def run():
            fn().backward(gout)
            for t in leaves:
                t.grad = None
        return run

    res = {"batch": label, "events": nb, "nodes": N, "min_nodes": min(lengths), "max_nodes": max(lengths), "F": F,
           "steps": steps}
    with torch.no_grad():
        res["graph_norm_max_abs_diff"] = float((gn(x, batch) - composed_graph_norm(gn, x, batch, nb)).abs().max())
        res["layer_norm_max_abs_diff"] = float((ln(x, batch) - composed_layer_norm(ln, x, batch, nb)).abs().max())
    t = alternate({"graph_norm_fused": step(lambda: gn(xx, batch), gn),
                   "graph_norm_composed": step(lambda: composed_graph_norm(gn, xx, batch, nb), gn),
                   "layer_norm_fused": step(lambda: ln(xx, batch), ln),
                   "layer_norm_composed": step(lambda: composed_layer_norm(ln, xx, batch, nb), ln),
                   "batch_norm": step(lambda: bn(xx), bn)}, steps, warmup, dev)
    names = ("event_moments", "event_dots", "event_affine")
    res["kernels_us"] = {"graph_norm": bracket(names, step(lambda: gn(xx, batch), gn), steps, dev),
                         "layer_norm": bracket(names, step(lambda: ln(xx, batch), ln), steps, dev)}
    floor_us = 5 * N * F * 4 / COPY_RATE * 1e6
    res["floor_us"] = round(floor_us, 2)
    for name, v in t.items():
        q = statistics.quantiles(v, n=4)
        res[name + "_us"] = round(statistics.median(v) * 1e3, 2)
        res[name + "_quartiles_us"] = [round(q[0] * 1e3, 2), round(q[2] * 1e3, 2)]
    for lay in ("graph_norm", "layer_norm"):
        res[lay + "_ratio"] = round(res[lay + "_composed_us"] / res[lay + "_fused_us"], 2)
        res[lay + "_floor_fraction"] = round(floor_us / res[lay + "_fused_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("event_norm_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for label, lengths in (("64x4500", [4500] * B), ("ragged 500-8000", ragged_lengths())):
        line = run_batch(label, lengths, a.steps, a.warmup, dev)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""Forward + backward time of one EdgeConv with a single Linear(64, 32) message at 64 x 4 500 nodes, by aggregation and
route: the fused routes for max, add and mean (csrc/edgeconv.hip, csrc/edgeconv_sum.hip) against the generic route for
add and mean (edge features, nn over E rows, segment sum), which nn = Sequential(Linear(64, 32), Identity()) forces.

    python tools/edgeconv_sum_step.py [--graphs knn radius] [--steps 30] [--warmup 5] [--json OUT]

knn: DynamicEdgeConv with k = 16 (the graph is rebuilt inside every step, as in the layer itself).  radius: EdgeConv over
a static radius_graph(r = 0.4, max_num_neighbors = 255, self loops) of uniform (eta, phi) in [-2.5, 2.5] x [-pi, pi],
built once.  One JSON line per (graph, aggr, route): median and mean of the per-step device time (HIP events around
forward + backward), the edge count, and the peak memory growth of one step."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402

VARIANTS = [("max", "fused"), ("add", "fused"), ("mean", "fused"), ("add", "generic"), ("mean", "generic")]


def make_inputs(B, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * n, 32, generator=g).to(dev)
    pos = torch.rand(B * n, 2, generator=g)
    pos[:, 0] = pos[:, 0] * 5.0 - 2.5
    pos[:, 1] = (pos[:, 1] * 2.0 - 1.0) * math.pi
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, ptr, B, max_nodes=n, min_nodes=n)
    return x, pos.to(dev), batch


def make_conv(graph, aggr, route, dev):
    torch.manual_seed(1)
    lin = torch.nn.Linear(64, 32)
    nn = torch.nn.Sequential(lin) if route == "fused" else torch.nn.Sequential(lin, torch.nn.Identity())
    conv = dm.DynamicEdgeConv(nn, k=16, aggr=aggr) if graph == "knn" else dm.EdgeConv(nn, aggr=aggr)
    return conv.to(dev)


def time_variant(conv, x, arg, g, steps, warmup, dev):
    xx = x.detach().clone().requires_grad_(True)
    times = []
    for it in range(warmup + steps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        conv(xx, arg).backward(g)
        b.record()
        if it >= warmup:
            times.append((a, b))
        xx.grad = None
        conv.zero_grad(set_to_none=True)
    torch.cuda.synchronize(dev)
    ms = [a.elapsed_time(b) for a, b in times]
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.max_memory_allocated(dev)
    conv(xx, arg).backward(g)
    torch.cuda.synchronize(dev)
    return ms, torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="+", choices=["knn", "radius"], default=["knn", "radius"])
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=4500)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, pos, batch = make_inputs(a.events, a.nodes, dev)
    g = torch.randn(x.shape[0], 32, generator=torch.Generator().manual_seed(2)).to(dev)
    lines = []
    for graph in a.graphs:
        if graph == "knn":
            arg = batch
            E = x.shape[0] * 16
        else:
            arg = dm.radius_graph(pos, 0.4, batch, loop=True, max_num_neighbors=255)
            E = int(arg.shape[1])
        for aggr, route in VARIANTS:
            conv = make_conv(graph, aggr, route, dev)
            ms, mem = time_variant(conv, x, arg, g, a.steps, a.warmup, dev)
            line = {"graph": graph, "aggr": aggr, "route": route, "events": a.events, "nodes": a.nodes, "edges": E,
                    "steps": a.steps, "median_ms": round(statistics.median(ms), 4),
                    "mean_ms": round(statistics.fmean(ms), 4), "min_ms": round(min(ms), 4),
                    "peak_growth_mb": round(mem / 2**20, 1)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

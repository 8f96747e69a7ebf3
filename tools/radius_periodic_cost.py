"""What the periodic phi of radius_graph(..., period=[None, 2 pi]) costs at the benchmark's shape (64 x 4500 events).

Alternated in one process, timed with device events:
  - the radius_table build, plain and periodic (median of --builds each);
  - the mean degree of each table;
  - the static-table training step as `bench.py --graph static-table` assembles it (eager, FlatAdamW, registered
    batch), once with each table (median of --steps each, in alternating blocks).
Prints one JSON line.  Usage: python tools/radius_periodic_cost.py [--builds 400] [--steps 200]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import deepmetv2_amd as dm
from deepmetv2_amd import synth
from deepmetv2_amd.model import Net
from deepmetv2_amd.optim import FlatAdamW
from deepmetv2_amd.parallel import FlatModule, GradSync, train_step

PERIOD = [None, 2 * math.pi]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=4500)
    ap.add_argument("--builds", type=int, default=400)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--block", type=int, default=10, help="steps per alternating block")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [args.nodes] * args.events
    x, y, batch, ptr = synth.make_events(sizes, seed=1234, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    etaphi = torch.cat([x[:, 3][:, None], torch.atan2(x[:, 1], x[:, 0])[:, None]], dim=1)     # train.py:45-48

    def table(period):
        return dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255, period=period)

    # builds, alternated
    times = {"plain": [], "periodic": []}
    for _ in range(20):
        table(None); table(PERIOD)
    torch.cuda.synchronize()
    for i in range(args.builds):
        for name, period in (("plain", None), ("periodic", PERIOD)) if i % 2 == 0 else (("periodic", PERIOD), ("plain", None)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); table(period); b.record()
            times[name].append((a, b))
    torch.cuda.synchronize()
    build_us = {k: statistics.median(a.elapsed_time(b) for a, b in v) * 1e3 for k, v in times.items()}
    deg = {k: float(table(p).cnt.float().mean()) for k, p in (("plain", None), ("periodic", PERIOD))}

    # the static-table training step with each table
    torch.manual_seed(0)
    model = Net(8, 3, graph="static", k=16).to(dev).train()
    flat = FlatModule(model)
    sync = GradSync(flat)
    opt = FlatAdamW([flat.flat_param], lr=1e-3)

    def step(period):
        return train_step(model, flat, sync, opt, x, y, batch, ptr, edge_index=table(period))

    for _ in range(10):
        step(None); step(PERIOD)
    torch.cuda.synchronize()
    st = {"plain": [], "periodic": []}
    blocks = max(1, args.steps // args.block)
    for i in range(blocks):
        order = (("plain", None), ("periodic", PERIOD)) if i % 2 == 0 else (("periodic", PERIOD), ("plain", None))
        for name, period in order:
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.block + 1)]
            evs[0].record()
            for s in range(args.block):
                step(period)
                evs[s + 1].record()
            st[name].append(evs)
    torch.cuda.synchronize()
    step_ms = {k: statistics.median(e[s].elapsed_time(e[s + 1]) for e in v for s in range(args.block)) for k, v in st.items()}
    out = {
        "shape": f"{args.events} x {args.nodes}", "r": 0.4, "max_num_neighbors": 255, "period": "[None, 2 pi]",
        "build_us_median": {k: round(v, 1) for k, v in build_us.items()},
        "build_ratio": round(build_us["periodic"] / build_us["plain"], 3),
        "builds_each": args.builds,
        "mean_degree": {k: round(v, 2) for k, v in deg.items()},
        "degree_ratio": round(deg["periodic"] / deg["plain"], 4),
        "static_table_step_ms_median": {k: round(v, 4) for k, v in step_ms.items()},
        "step_ratio": round(step_ms["periodic"] / step_ms["plain"], 4),
        "steps_each": blocks * args.block,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What the periodic phi of knn_table(..., period=[None, 2 pi]) costs at the benchmark's shape (64 x 4500 events), k = 16,
loop=True, registered batch.

Alternated in one process, timed with device events:
  - the kNN build in (eta, phi), plain D = 2 and periodic (median of --builds each), and the periodic radius build
    (r = 0.4, 255 neighbours) for context;
  - the static-table training step as `bench.py --graph static-table` assembles it (eager, FlatAdamW, registered
    batch), once over the periodic radius table and once over the periodic k = 16 kNN table (median of --steps each,
    in alternating blocks).
Prints one JSON line (and writes it to --out if given).  Usage: python tools/knn_periodic_cost.py [--builds 400]
[--steps 200] [--out FILE]"""
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
K = 16


def _median_us(pairs):
    return statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=4500)
    ap.add_argument("--builds", type=int, default=400)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--block", type=int, default=10, help="steps per alternating block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [args.nodes] * args.events
    x, y, batch, ptr = synth.make_events(sizes, seed=1234, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    etaphi = torch.cat([x[:, 3][:, None], torch.atan2(x[:, 1], x[:, 0])[:, None]], dim=1)     # train.py:45-48

    builds = {
        "knn_plain": lambda: dm.knn_table(etaphi, K, batch, loop=True),
        "knn_periodic": lambda: dm.knn_table(etaphi, K, batch, loop=True, period=PERIOD),
        "radius_periodic": lambda: dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255,
                                                   period=PERIOD),
    }
    names = list(builds)
    for _ in range(20):
        for n in names:
            builds[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for i in range(args.builds):
        for n in (names if i % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); builds[n](); b.record()
            times[n].append((a, b))
    torch.cuda.synchronize()
    build_us = {n: _median_us(v) for n, v in times.items()}
    seam = etaphi[:, 1].abs() > math.pi - 0.4
    plain_t, per_t = builds["knn_plain"](), builds["knn_periodic"]()
    changed = float((plain_t.nbr[seam] != per_t.nbr[seam]).any(dim=1).float().mean())

    # the static-table training step over each table
    torch.manual_seed(0)
    model = Net(8, 3, graph="static", k=K).to(dev).train()
    flat = FlatModule(model)
    sync = GradSync(flat)
    opt = FlatAdamW([flat.flat_param], lr=1e-3)
    graphs = {"radius_periodic": builds["radius_periodic"], "knn_periodic": builds["knn_periodic"]}

    def step(name):
        return train_step(model, flat, sync, opt, x, y, batch, ptr, edge_index=graphs[name]())

    for _ in range(10):
        for n in graphs:
            step(n)
    torch.cuda.synchronize()
    st = {n: [] for n in graphs}
    order = list(graphs)
    blocks = max(1, args.steps // args.block)
    for i in range(blocks):
        for n in (order if i % 2 == 0 else order[::-1]):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.block + 1)]
            evs[0].record()
            for s in range(args.block):
                step(n)
                evs[s + 1].record()
            st[n].append(evs)
    torch.cuda.synchronize()
    step_ms = {k: statistics.median(e[s].elapsed_time(e[s + 1]) for e in v for s in range(args.block)) for k, v in st.items()}
    out = {
        "shape": f"{args.events} x {args.nodes}", "k": K, "loop": True, "period": "[None, 2 pi]",
        "build_us_median": {k: round(v, 1) for k, v in build_us.items()},
        "knn_build_ratio": round(build_us["knn_periodic"] / build_us["knn_plain"], 3),
        "builds_each": args.builds,
        "seam_rows_changed": round(changed, 4),
        "static_table_step_ms_median": {k: round(v, 4) for k, v in step_ms.items()},
        "step_ratio_knn_over_radius": round(step_ms["knn_periodic"] / step_ms["radius_periodic"], 4),
        "steps_each": blocks * args.block,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

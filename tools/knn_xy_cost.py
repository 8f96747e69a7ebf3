"""What the two-set builders cost next to the one-set builds of the same pairs (64 x 4500 events unless told otherwise).

Alternated in one process, timed with device events, batches registered (no host sync in either build):
  d2        (a) knn_table(etaphi, 16, batch, period=[None, 2 pi])   -- always the exact kernel
            (b) knn_xy_table(etaphi, etaphi.clone(), 16, batch, batch.clone(), period=...)   -- the same pairs
  d32       (a) knn_table(x32, 32, batch)  -- k = 32 is outside the matrix-core path: the exact kernel
            (b) knn_xy_table(x32, x32.clone(), 32, batch, batch.clone())
  radius    (a) radius_table([phi, eta], 0.4, loop=True, 255 wide, period=[2 pi, None])  -- the all-pairs periodic build
            (b) radius_xy_table of the same points on both sides
  unbalanced shapes of the two-set kNN (D = 2, k = 16): 4500 queries x 64 candidates per event, and the reverse.
Prints one JSON line with median / p10 / p90 in microseconds and pairs per second (and writes it to --out if given).
Usage: python tools/knn_xy_cost.py [--builds 300] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import deepmetv2_amd as dm


def _events(sizes, D, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(sizes), D, generator=g)
    if D == 2:      # (eta, phi)
        x = torch.stack([(torch.rand(sum(sizes), generator=g) - 0.5) * 6, (torch.rand(sum(sizes), generator=g) - 0.5) * 2 * math.pi], 1)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    return x.to(dev), batch


def _time(builds, n, warm=20):
    names = list(builds)
    for _ in range(warm):
        for name in names:
            builds[name]()
    torch.cuda.synchronize()
    ev = {name: [] for name in names}
    for _ in range(n):
        for name in names:              # alternated
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            builds[name]()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for name in names:
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[name])
        out[name] = {"median_us": round(statistics.median(t), 1), "p10_us": round(t[len(t) // 10], 1),
                     "p90_us": round(t[(9 * len(t)) // 10], 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=4500)
    ap.add_argument("--builds", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n = args.events, args.nodes
    res = {"events": B, "nodes": n, "builds": args.builds}

    def with_rate(t, pairs):
        for v in t.values():
            v["gpairs_per_s"] = round(pairs / v["median_us"] * 1e-3, 1)
        return t

    per = [None, 2 * math.pi]
    x2, b2 = _events([n] * B, 2, 1, dev)
    x2c, b2c = x2.clone(), b2.clone()
    dm.register_batch(b2c, dm.graph.batch_info(b2, x2.shape[0], dev).ptr, B, max_nodes=n, min_nodes=n)
    res["d2_k16"] = with_rate(_time({
        "self": lambda: dm.knn_table(x2, 16, b2, loop=True, period=per),
        "xy": lambda: dm.knn_xy_table(x2, x2c, 16, b2, b2c, period=per)}, args.builds), B * n * n)

    x32, b32 = _events([n] * B, 32, 2, dev)
    x32c, b32c = x32.clone(), b32.clone()
    dm.register_batch(b32c, dm.graph.batch_info(b32, x32.shape[0], dev).ptr, B, max_nodes=n, min_nodes=n)
    res["d32_k32"] = with_rate(_time({
        "self": lambda: dm.knn_table(x32, 32, b32, loop=True),
        "xy": lambda: dm.knn_xy_table(x32, x32c, 32, b32, b32c)}, max(args.builds // 3, 20)), B * n * n)

    pe = x2.flip(1).contiguous()            # [phi, eta]: the periodic coordinate first -> the all-pairs radius build
    pec = pe.clone()
    per_pe = [2 * math.pi, None]
    res["radius_r0.4_255"] = with_rate(_time({
        "self": lambda: dm.radius_table(pe, 0.4, b2, loop=True, max_num_neighbors=255, int32_rows=True, period=per_pe),
        "xy": lambda: dm.radius_xy_table(pe, pec, 0.4, b2, b2c, 255, period=per_pe)}, args.builds), B * n * n)

    few, bf = _events([64] * B, 2, 3, dev)
    res["unbalanced_d2_k16"] = with_rate(_time({
        "4500q_x_64c": lambda: dm.knn_xy_table(few, x2, 16, bf, b2),
        "64q_x_4500c": lambda: dm.knn_xy_table(x2, few, 16, b2, bf)}, args.builds), B * n * 64)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

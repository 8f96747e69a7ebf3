"""Forward + backward time of PointNetConv's fused route (csrc/pointnet.hip) against the generic route of the same layer
(DMET_POINTNET=0: torch indexing over the edge list, local_nn over E rows, segment max) and against the two-set EdgeConv
that stood in for it before (nn([x_i || x_j - x_i]) over the centres' features: another layer, the same traffic).

    python tools/pointnet_step.py [--shapes 64x4500] [--ratio 0.25] [--steps 50] [--warmup 10] [--repeats 5] [--json OUT]

One JSON line per shape: B events of n nodes, ceil(ratio n) centres per event from fps, knn_xy_table k = 16 from the
nodes onto the centres, F = 32 features, D = 2 coordinates, local_nn = Linear(34, 64) - ReLU - Linear(64, 64).  The graph is
built once, outside the timed region.  The three variants alternate inside one loop; `*_ms` are medians of the per-step
device time (HIP events) over all repeats, `*_medians` the median of each repeat, `spread_ms` the largest distance between
two medians of one variant: what a difference between two variants has to exceed to mean anything.  `kernels`: the
HIP-event brackets of the two native calls."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native  # noqa: E402

F, D, H1, H2, K = 32, 2, 64, 64, 16


def make_inputs(B, n, ratio, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    pos = torch.randn(B * n, D, generator=g).to(dev)
    x = torch.randn(B * n, F, generator=g).to(dev)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, ptr, B, max_nodes=n, min_nodes=n)
    idx = dm.fps(pos, batch, ratio, random_start=False)
    m = math.ceil(n * ratio)
    assert idx.numel() == B * m
    pos_c, batch_c = pos[idx].contiguous(), batch[idx].contiguous()
    dm.register_batch(batch_c, torch.arange(0, (B + 1) * m, m, dtype=torch.int64, device=dev), B, max_nodes=m, min_nodes=m)
    return x, pos, pos_c, batch, batch_c, idx


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


def run_shape(B, n, ratio, steps, warmup, repeats, dev):
    x, pos, pos_c, batch, batch_c, idx = make_inputs(B, n, ratio, dev)
    torch.manual_seed(0)
    local_nn = torch.nn.Sequential(torch.nn.Linear(F + D, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2)).to(dev)
    conv = dm.PointNetConv(local_nn, add_self_loops=False)
    stand_in = dm.EdgeConv(torch.nn.Sequential(torch.nn.Linear(2 * F, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2)).to(dev),
                           aggr="max")
    table = dm.knn_xy_table(pos, pos_c, K, batch, batch_c)
    table.reverse()
    table.edge_list()
    Nt = pos_c.shape[0]
    g = torch.randn(Nt, H2, generator=torch.Generator().manual_seed(2)).to(dev)
    xx = x.clone().requires_grad_(True)
    pp, pc = pos.clone().requires_grad_(True), pos_c.clone().requires_grad_(True)
    x_c = x[idx].contiguous()

    def clear(mod):
        xx.grad = pp.grad = pc.grad = None
        for p in mod.parameters():
            p.grad = None

    def fused():
        conv((xx, None), (pp, pc), table).backward(g)
        clear(conv)

    def generic():
        os.environ["DMET_POINTNET"] = "0"
        try:
            conv((xx, None), (pp, pc), table).backward(g)
        finally:
            del os.environ["DMET_POINTNET"]
        clear(conv)

    def edgeconv():
        stand_in((xx, x_c), table).backward(g)
        clear(stand_in)

    fns = {"fused": fused, "generic": generic, "edgeconv_stand_in": edgeconv}
    runs = [alternate(fns, steps, warmup, dev) for _ in range(repeats)]
    out = {"events": B, "nodes": n, "centres": Nt // B, "edges": Nt * K, "F": F, "D": D, "H1": H1, "H2": H2, "k": K,
           "steps": steps, "repeats": repeats}
    for name in fns:
        meds = [statistics.median(r[name]) for r in runs]
        out[f"{name}_ms"] = round(statistics.median([v for r in runs for v in r[name]]), 4)
        out[f"{name}_medians"] = [round(m, 4) for m in meds]
        out[f"{name}_spread_ms"] = round(max(meds) - min(meds), 4)
    out["spread_ms"] = max(out[f"{name}_spread_ms"] for name in fns)
    out["generic_over_fused"] = round(out["generic_ms"] / out["fused_ms"], 2)
    out["edgeconv_over_fused"] = round(out["edgeconv_stand_in_ms"] / out["fused_ms"], 2)

    # the two native calls on their own brackets (a run of its own: every bracket is two more stream commands)
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, {"pointnet_fwd", "pointnet_bwd"}
    for _ in range(steps):
        fused()
    torch.cuda.synchronize(dev)
    summary = _native.timer.summary()
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()
    flops = 2.0 * Nt * K * H1 * H2
    out["kernels"] = {name: {"mean_ms": round(summary[name][1], 4)} for name in ("pointnet_fwd", "pointnet_bwd")}
    out["kernels"]["pointnet_fwd"]["per_entry_product_tflops"] = round(flops / (summary["pointnet_fwd"][1] * 1e-3) / 1e12, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500"])
    ap.add_argument("--ratio", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointnet_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes:
        B, n = (int(v) for v in shape.split("x"))
        line = run_shape(B, n, a.ratio, a.steps, a.warmup, a.repeats, dev)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

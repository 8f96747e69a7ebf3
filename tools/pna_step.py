"""Forward + backward time of multi_aggregate (csrc/multi_aggr.hip) with PNA's [mean, min, max, std] against the composed
route over the same table -- x.index_select plus this package's scatter_mean / scatter_min / scatter_max and a standard
deviation from two scatter_mean calls -- and of the PNAConv layer, fused against DMET_PNA=0.

    python tools/pna_step.py [--shapes 64x4500] [--k 16] [--steps 30] [--warmup 5] [--layer-steps 8] [--json OUT]

One JSON line per shape: B events of n nodes, a kNN table of width k (self loops), F = 64 features.  `aggregate_*`:
forward + backward over a prebuilt table and reverse index (fused) or the table's prebuilt edge list (composed; every
scatter call still groups its index, as its public form does), the two taking turns inside one loop, medians of the
per-step device time (HIP events).  `max_abs_diff`: the two routes' outputs against each other at the timed size.
`kernels`: the HIP-event brackets of the two native calls.  `layer_*`: PNAConv(64, 64, towers=4, three scalers), forward
+ backward, the fused route and the generic one (per-edge messages) on the same weights."""
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

F, D = 64, 2
AGGRS = ("mean", "min", "max", "std")


def composed(x, src, index, N):
    """[N, 4, F]: the same four statistics from the package's scatter family over the [E, F] messages."""
    msg = x.index_select(0, src)
    mean = dm.scatter_mean(msg, index, dim=0, dim_size=N)
    mn = dm.scatter_min(msg, index, dim=0, dim_size=N)[0]
    mx = dm.scatter_max(msg, index, dim=0, dim_size=N)[0]
    var = dm.scatter_mean(msg * msg, index, dim=0, dim_size=N) - mean * mean
    std = var.clamp(min=1e-5).sqrt()
    std = std.masked_fill(std <= math.sqrt(1e-5), 0.0)
    return torch.stack([mean, mn, mx, std], dim=1)


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


def run_shape(B, n, k, steps, warmup, layer_steps, dev):
    g = torch.Generator().manual_seed(0)
    N = B * n
    pos = torch.randn(N, D, generator=g).to(dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev), B, max_nodes=n, min_nodes=n)
    table = dm.knn_table(pos, k, batch, loop=True)
    table.reverse()
    edges = table.edge_list()
    src, index = edges.src.long(), edges.tgt.long()
    x = torch.randn(N, F, generator=g).to(dev)
    gout = torch.randn(N, len(AGGRS), F, generator=g).to(dev)
    xx = x.clone().requires_grad_(True)

    def step(fn, grad):
        def run():
            fn().backward(grad)
            xx.grad = None
        return run

    with torch.no_grad():
        diff = float((dm.multi_aggregate(x, table, AGGRS)[0] - composed(x, src, index, N)).abs().max())
    agg = alternate({"fused": step(lambda: dm.multi_aggregate(xx, table, AGGRS)[0], gout),
                     "composed": step(lambda: composed(xx, src, index, N), gout)}, steps, warmup, dev)

    # the two native calls on their own brackets (a run of its own: every bracket is two more stream commands)
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, {"multi_aggr_fwd", "multi_aggr_bwd"}
    one = step(lambda: dm.multi_aggregate(xx, table, AGGRS)[0], gout)
    for _ in range(steps):
        one()
    torch.cuda.synchronize(dev)
    kernels = {name: round(ms, 4) for name, (_count, ms) in _native.timer.summary().items()}
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()

    # the layer: in = out = 64, four towers, on the same table
    torch.manual_seed(1)
    deg = torch.zeros(k + 1)
    deg[k] = N
    conv = dm.PNAConv(F, F, list(AGGRS), ["identity", "amplification", "attenuation"], deg, towers=4).to(dev)
    gl = torch.randn(N, F, generator=g).to(dev)

    def layer(flag):
        def run():
            os.environ["DMET_PNA"] = flag
            conv(xx, table).backward(gl)
            xx.grad = None
            conv.zero_grad(set_to_none=True)
        return run
    lay = alternate({"fused": layer("1"), "generic": layer("0")}, layer_steps, 2, dev)
    os.environ.pop("DMET_PNA", None)

    def med(v):
        return round(statistics.median(v), 4)
    return {"events": B, "nodes": n, "k": k, "F": F, "edges": N * k, "aggrs": list(AGGRS), "steps": steps,
            "aggregate_fused_ms": med(agg["fused"]), "aggregate_composed_ms": med(agg["composed"]),
            "aggregate_ratio": round(statistics.median(agg["composed"]) / statistics.median(agg["fused"]), 2),
            "max_abs_diff": diff, "kernels": kernels,
            "layer_fused_ms": med(lay["fused"]), "layer_generic_ms": med(lay["generic"]),
            "layer_ratio": round(statistics.median(lay["generic"]) / statistics.median(lay["fused"]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500"])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layer-steps", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pna_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes:
        B, n = (int(v) for v in shape.split("x"))
        line = run_shape(B, n, a.k, a.steps, a.warmup, a.layer_steps, dev)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

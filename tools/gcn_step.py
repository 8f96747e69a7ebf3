"""Forward + backward time of weighted_aggregate (csrc/weighted_sum.hip) against the torch composition over the same
graph -- x.index_select, the [E, F] product with the weights and index_add_ -- of the unweighted form against
multi_aggregate(x, table, ['sum']) (the same gather), and of GCNConv(64, 64), fused against the same layer composed from
torch operators.

    python tools/gcn_step.py [--shapes 64x4500] [--k 16] [--steps 30] [--warmup 5] [--json OUT]

One JSON line per shape: B events of n nodes, a kNN table of width k (self loops), F = 64 features.  `weighted_*`: forward
+ backward with gradients to x and to the weights, over a prebuilt table and reverse index (fused) or the table's
prebuilt edge list (composed).  `plain_*`: no weights, gradient to x.  `layer_*`: GCNConv with edge weights, gradients to
x, the weights and the parameters; every row of the table holds its own node, so the composed layer needs no self-loop
insertion (that favours it).  The variants of a pair take turns inside one loop; medians of the per-step device time
(HIP events).  `max_abs_diff`: the two routes' outputs against each other at the timed size.  `kernels`: the HIP-event
brackets of the native calls -- the forward, and the backward run once for the gradient of x alone (the by-source
kernel) and once for the gradient of the weights alone (the by-target kernel)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native  # noqa: E402

F, D = 64, 2


def composed(x, w, src, tgt, N):
    """[N, F]: index_select, the per-edge product, index_add_ (float atomics)."""
    msg = x.index_select(0, src)
    if w is not None:
        msg = msg * w.view(-1, 1)
    return torch.zeros((N, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, tgt, msg)


def composed_gcn(conv, x, w, src, tgt, N):
    """GCNConv from torch operators over a graph that already holds every self loop: gcn_norm's degree and normalised
    [E] weight, then the weighted sum of lin(x)."""
    deg = torch.zeros(N, dtype=x.dtype, device=x.device).index_add_(0, tgt, w)
    dinv = deg.pow(-0.5)
    dinv = dinv.masked_fill(dinv == float("inf"), 0.0)
    return composed(conv.lin(x), dinv[src] * w * dinv[tgt], src, tgt, N) + conv.bias


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
    """{name: ms per call} of the native calls `names` over `steps` runs of fn (a run of its own: every bracket is two
    more stream commands)."""
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, set(names)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    out = {name: round(ms, 4) for name, (_count, ms) in _native.timer.summary().items()}
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()
    return out


def run_shape(B, n, k, steps, warmup, dev):
    g = torch.Generator().manual_seed(0)
    N = B * n
    pos = torch.randn(N, D, generator=g).to(dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev), B, max_nodes=n, min_nodes=n)
    table = dm.knn_table(pos, k, batch, loop=True)
    table.reverse()
    edges = table.edge_list()
    src, tgt = edges.src.long(), edges.tgt.long()
    if edges.num_edges != N * k:        # every slot holds an entry: the list's order is the table's, one weight vector serves both
        raise SystemExit("gcn_step.py: the kNN table has short rows; the composed routes need the full table")
    x =torch.randn(N, F, generator=g).to(dev)
    w = (0.1 + torch.rand(N * k, generator=g)).to(dev)
    gout = torch.randn(N, F, generator=g).to(dev)
    xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

    def step(fn, leaves):
        def run():
            fn().backward(gout)
            for t in leaves:
                t.grad = None
        return run

    res = {"events": B, "nodes": n, "k": k, "F": F, "edges": edges.num_edges, "steps": steps}
    with torch.no_grad():
        res["weighted_max_abs_diff"] = float((dm.weighted_aggregate(x, table, w) - composed(x, w, src, tgt, N)).abs().max())
        res["plain_max_abs_diff"] = float((dm.weighted_aggregate(x, table)
                                           - dm.multi_aggregate(x, table, ["sum"])[0][:, 0]).abs().max())
    t = alternate({"fused": step(lambda: dm.weighted_aggregate(xx, table, ww), (xx, ww)),
                   "composed": step(lambda: composed(xx, ww, src, tgt, N), (xx, ww))}, steps, warmup, dev)
    p = alternate({"weighted_sum": step(lambda: dm.weighted_aggregate(xx, table), (xx,)),
                   "multi_aggr": step(lambda: dm.multi_aggregate(xx, table, ["sum"])[0][:, 0], (xx,)),
                   "composed": step(lambda: composed(xx, None, src, tgt, N), (xx,))}, steps, warmup, dev)

    torch.manual_seed(1)
    conv = dm.GCNConv(F, F).to(dev)
    leaves = (xx, ww) + tuple(conv.parameters())
    with torch.no_grad():
        res["layer_max_abs_diff"] = float((conv(x, table, w) - composed_gcn(conv, x, w, src, tgt, N)).abs().max())
    lay = alternate({"fused": step(lambda: conv(xx, table, ww), leaves),
                     "composed": step(lambda: composed_gcn(conv, xx, ww, src, tgt, N), leaves)}, steps, warmup, dev)

    names = ("weighted_sum_fwd", "weighted_sum_bwd")
    both = bracket(names, step(lambda: dm.weighted_aggregate(xx, table, ww), (xx, ww)), steps, dev)
    only_x = bracket(names, step(lambda: dm.weighted_aggregate(xx, table, w), (xx,)), steps, dev)
    only_w = bracket(names, step(lambda: dm.weighted_aggregate(x, table, ww), (ww,)), steps, dev)
    res["kernels"] = {"fwd": both.get("weighted_sum_fwd"), "bwd_both": both.get("weighted_sum_bwd"),
                      "bwd_x": only_x.get("weighted_sum_bwd"), "bwd_w": only_w.get("weighted_sum_bwd")}

    def med(v):
        return round(statistics.median(v), 4)

    def spread(v):
        q = statistics.quantiles(v, n=4)
        return [round(q[0], 4), round(q[2], 4)]
    res.update({"weighted_fused_ms": med(t["fused"]), "weighted_composed_ms": med(t["composed"]),
                "weighted_ratio": round(statistics.median(t["composed"]) / statistics.median(t["fused"]), 2),
                "plain_weighted_sum_ms": med(p["weighted_sum"]), "plain_multi_aggr_ms": med(p["multi_aggr"]),
                "plain_composed_ms": med(p["composed"]),
                "plain_weighted_sum_quartiles": spread(p["weighted_sum"]), "plain_multi_aggr_quartiles": spread(p["multi_aggr"]),
                "layer_fused_ms": med(lay["fused"]), "layer_composed_ms": med(lay["composed"]),
                "layer_ratio": round(statistics.median(lay["composed"]) / statistics.median(lay["fused"]), 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500"])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcn_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes:
        B, n = (int(v) for v in shape.split("x"))
        line = run_shape(B, n, a.k, a.steps, a.warmup, dev)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

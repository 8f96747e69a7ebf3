"""Forward + backward time of TopKPooling(64, 0.5) (csrc/select.hip) over a k = 16 neighbour table and over the table's
int64 [2, E] edge index, and of `topk` alone, each against the same formulas composed from torch operators: a
composite-key torch.sort for the ranking, indexing for the gate, mask + nonzero for the edges.

    python tools/select_step.py [--steps 30] [--warmup 5] [--json OUT]

Two batches of the same total, F = 64 fp32: 64 events of 4500 nodes, and 64 events of 500 to 8000 nodes (seeded, adjusted
to the same 288 000).  One JSON line per batch.  The variants take turns inside one loop; medians of the per-step device
time (HIP events; a step that reads the device -- the [2, E] routes and the composed ones read a size -- includes that
wait).  Gradients to x and to the layer's weight.  `max_abs_diff`: native against composed outputs at the timed size;
`perm_equal`: the two rankings agree (the Gaussian scores are distinct).  `kernels_us`: HIP-event brackets of the native
calls, per launch, in a run of their own (`filter_edges` holds its host read of E').  The table is built at random inside the events
(the pooling does not look at geometry), with 10 % holes."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native  # noqa: E402

F, B, K, TOTAL, RATIO = 64, 64, 16, 64 * 4500, 0.5


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


def composed_topk(score, ratio, batch, ptr):
    """perm by one sort over a composite key: a stable descending sort by score, then a stable sort by event."""
    deg = ptr[1:] - ptr[:-1]
    m = torch.ceil(deg.to(torch.float32) * ratio).to(torch.int64)
    order = torch.sort(score, descending=True, stable=True).indices
    order = order[torch.sort(batch[order], stable=True).indices]
    rank = torch.arange(score.numel(), device=score.device) - ptr[:-1][batch]
    return order[rank < m[batch]]


def composed_pool(layer, x, edge_index, batch, ptr):
    w = layer.select.weight
    score = torch.tanh((x * w).sum(-1) / w.norm(p=2, dim=-1))
    perm = composed_topk(score.detach(), RATIO, batch, ptr)
    out = x[perm] * score[perm].view(-1, 1)
    node_map = torch.full((x.shape[0],), -1, dtype=torch.int64, device=x.device)
    node_map[perm] = torch.arange(perm.numel(), device=x.device)
    row, col = node_map[edge_index[0]], node_map[edge_index[1]]
    keep = ((row >= 0) & (col >= 0)).nonzero().view(-1)
    return out, torch.stack([row[keep], col[keep]]), batch[perm], perm, score[perm]


def _sorted_edges(ei):
    """The edges as sorted (target, source) keys: the table lists them by pooled row, the edge index in the caller's order."""
    return torch.sort(ei[1] * (int(ei.max()) + 1 if ei.numel() else 1) + ei[0]).values


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
    """{kernel: us per launch}: HIP-event brackets of the native calls, in a run of their own."""
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
    N, nb = sum(lengths), len(lengths)
    ptr_h = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(lengths).cumsum(0)])
    ptr = ptr_h.to(dev)
    batch_h = torch.repeat_interleave(torch.arange(nb), torch.tensor(lengths))
    batch = batch_h.to(dev)
    dm.register_batch(batch, ptr, nb, max_nodes=max(lengths), min_nodes=min(lengths))
    x = torch.randn(N, F, generator=g).to(dev)
    lo, n = ptr_h[:-1][batch_h].view(-1, 1), torch.tensor(lengths)[batch_h].view(-1, 1)
    nbr = ((torch.rand(N, K, generator=g) * n).long().clamp(max=n - 1) + lo).to(torch.int32)
    nbr[torch.rand(N, K, generator=g) < 0.1] = -1
    table = dm.NeighborTable(nbr.to(dev), ptr, dense=False, max_nodes=max(lengths))
    ok = nbr >= 0
    edge_index = torch.stack([nbr[ok].long(), torch.arange(N).view(-1, 1).expand(N, K)[ok]]).to(dev)
    xx = x.clone().requires_grad_(True)
    torch.manual_seed(2)
    layer = dm.TopKPooling(F, RATIO).to(dev)
    score = torch.randn(N, generator=g).to(dev)
    leaves = (xx,) + tuple(layer.parameters())

    def step(fn):
        def run():
            out = fn()
            out[0].backward(gout[: out[0].shape[0]])
            for t in leaves:
                t.grad = None
        return run

    res = {"batch": label, "events": nb, "nodes": N, "min_nodes": min(lengths), "max_nodes": max(lengths), "F": F, "k": K,
           "edges": int(edge_index.shape[1]), "steps": steps}
    with torch.no_grad():
        nat, comp = layer(x, edge_index, None, batch), composed_pool(layer, x, edge_index, batch, ptr)
        tab = layer(x, table, None, batch)
        res["perm_equal"] = bool(torch.equal(nat[4], comp[3])) and bool(torch.equal(tab[4], comp[3]))
        res["perm_equal_topk"] = bool(torch.equal(dm.topk(score, RATIO, batch), composed_topk(score, RATIO, batch, ptr)))
        res["x_max_abs_diff"] = float((nat[0] - comp[0]).abs().max())
        res["score_max_abs_diff"] = float((nat[5] - comp[4]).abs().max())
        res["edge_index_equal"] = bool(torch.equal(nat[1], comp[1]))
        res["table_edges_equal"] = bool(torch.equal(_sorted_edges(tab[1].edge_index()), _sorted_edges(comp[1])))
        res["pooled_nodes"], res["pooled_edges"] = int(nat[4].numel()), int(nat[1].shape[1])
    gout = torch.randn(N, F, generator=g).to(dev)
    t = alternate({"pool_table_native": step(lambda: layer(xx, table, None, batch)),
                   "pool_edges_native": step(lambda: layer(xx, edge_index, None, batch)),
                   "pool_edges_composed": step(lambda: composed_pool(layer, xx, edge_index, batch, ptr)),
                   "topk_native": lambda: dm.topk(score, RATIO, batch),
                   "topk_composed": lambda: composed_topk(score, RATIO, batch, ptr)}, steps, warmup, dev)
    names = ("topk", "select_rows", "select_rows_bwd", "filter_table", "filter_edges")
    res["kernels_us"] = {"pool_table": bracket(names, step(lambda: layer(xx, table, None, batch)), steps, dev),
                         "pool_edges": bracket(names, step(lambda: layer(xx, edge_index, None, batch)), steps, dev)}
    for name, v in t.items():
        q = statistics.quantiles(v, n=4)
        res[name + "_us"] = round(statistics.median(v) * 1e3, 2)
        res[name + "_quartiles_us"] = [round(q[0] * 1e3, 2), round(q[2] * 1e3, 2)]
    res["pool_table_ratio"] = round(res["pool_edges_composed_us"] / res["pool_table_native_us"], 2)
    res["pool_edges_ratio"] = round(res["pool_edges_composed_us"] / res["pool_edges_native_us"], 2)
    res["topk_ratio"] = round(res["topk_composed_us"] / res["topk_native_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_step.py measures on a GPU; none is visible")
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

"""Time of the edge matching (csrc/edge_match.hip) against the same round rule composed from torch operators, of
`EdgePooling` forward + backward, and -- for context -- of the fixed coarsening it replaces in the DynamicReductionNetwork
(normalized_cut_2d + graclus + max_pool_x) on the same graph.

    python tools/edge_pool_step.py [--steps 50] [--warmup 5] [--json OUT]

Two batches of the same total, a k = 16 knn_graph over 2-D positions, F = 64 fp32: 64 events of 4500 nodes, and 64 events
of 500 to 8000 nodes (seeded, adjusted to the same 288 000).  The scores are the layer's own (softmax by target + 0.5).
One JSON line per batch, and one for the worst case: ONE 4500-node path with strictly descending scores (n / 2 rounds,
one edge each), with its cost per round.  The variants take turns inside one loop; medians of the per-step device time
(HIP events; a step that reads from the device includes that wait).

  match_native      dmet_edge_match_f32 alone: one launch, every round of every event inside it
  match_composed    the same rule on the device from torch operators: scatter_reduce(amax) over int64 keys, one host check
                    per round (`any edge live?`) -- the only upstream-shaped alternative that stays on the device
  edge_pool_step    EdgePooling forward + backward
  graclus_step      normalized_cut_2d + graclus + max_pool_x forward + backward on the undirected graph (made outside the
                    loop), for context: another coarsening, not the same result
`match_us`: HIP-event bracket of the native launch in a run of its own.  `rounds`: of the native launch, per event.
`launches`: device kernels of one call (torch.profiler).  `host_reads`: synchronising calls of one call
(torch.cuda.set_sync_debug_mode).  `equal`: native and composed clusters agree at the timed size."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native, edge_pool  # noqa: E402
from deepmetv2_amd.graph import edge_list_from_edge_index  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from voxel_step import alternate, bracket, launches, ragged_lengths  # noqa: E402

F, B, K = 64, 64, 16


def order_key(score, ids):
    """The kernel's order as a non-negative int64 (the 32 order bits above 31 bits of -id)."""
    u = score.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    hi = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    hi = torch.where(nan, torch.full_like(hi, 0xFFFFFFFF), hi)
    return (hi << 31) | (0x7FFFFFFF - ids)


def composed_match(src, tgt, key, N):
    """(cluster[N], rounds): rounds of locally dominant edges from torch operators; one host check per round."""
    dev = src.device
    claimed = torch.zeros(N, dtype=torch.bool, device=dev)
    cluster = torch.arange(N, dtype=torch.int64, device=dev)
    low, none = torch.minimum(src, tgt), torch.full_like(src, N)
    rounds = 0
    while True:
        live = ~(claimed[src] | claimed[tgt])
        if not bool(live.any()):
            return cluster, rounds
        rounds += 1
        k = torch.where(live, key, torch.zeros_like(key))
        best = torch.zeros(N, dtype=torch.int64, device=dev).scatter_reduce_(0, src, k, "amax").scatter_reduce_(0, tgt, k, "amax")
        take = live & (best[src] == key) & (best[tgt] == key)
        lead = torch.where(take, low, none)
        cluster = torch.minimum(cluster, torch.full_like(cluster, N).scatter_reduce_(0, src, lead, "amin")
                                .scatter_reduce_(0, tgt, lead, "amin"))
        hit = take.to(torch.int32)
        claimed |= torch.zeros(N, dtype=torch.int32, device=dev).index_add_(0, src, hit).index_add_(0, tgt, hit) > 0


def host_reads(fn, dev):
    fn()
    torch.cuda.synchronize(dev)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return sum("called a synchronizing" in str(r.message) for r in rec)


def medians(t, res):
    for name, v in t.items():
        q = statistics.quantiles(v, n=4)
        res[name + "_us"] = round(statistics.median(v) * 1e3, 2)
        res[name + "_quartiles_us"] = [round(q[0] * 1e3, 2), round(q[2] * 1e3, 2)]


def match_only(res, g, score, ptr, src64, tgt64, N, steps, warmup, dev):
    """The native launch against the composed rounds on one grouped graph; fills res."""
    ids = torch.arange(src64.numel(), dtype=torch.int64, device=dev) if g.edges.perm is None else g.edges.perm.long()
    key = order_key(score, ids)

    def native():
        return _native._edge_match(g.edges.rowptr, g.src, g.edges.tgt, g.edges.perm, score, ptr, True)

    cluster, _partner, _edge, rounds, flags = native()
    composed, n_rounds = composed_match(src64, tgt64, key, N)
    r = rounds.cpu()
    res["equal"] = bool(torch.equal(cluster, composed)) and flags.cpu().tolist() == [0, 0, 0]
    res["rounds"] = {"max": int(r.max()), "min": int(r.min()), "mean": round(float(r.float().mean()), 2), "composed": n_rounds}
    res["clusters"] = int((cluster == torch.arange(N, device=dev)).sum())
    t = alternate({"match_native": native, "match_composed": lambda: composed_match(src64, tgt64, key, N)}, steps, warmup, dev)
    medians(t, res)
    res["match_us"] = bracket(("edge_match",), native, steps, dev).get("edge_match")
    res["match_ratio"] = round(res["match_composed_us"] / res["match_native_us"], 2)
    res["launches"] = {"match_native": launches(native, dev),
                       "match_composed": launches(lambda: composed_match(src64, tgt64, key, N), dev)}
    res["host_reads"] = {"match_native": host_reads(native, dev),
                         "match_composed": host_reads(lambda: composed_match(src64, tgt64, key, N), dev)}


def run_batch(label, lengths, steps, warmup, dev):
    g = torch.Generator().manual_seed(1)
    N, nb = sum(lengths), len(lengths)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(lengths).cumsum(0)]).to(dev)
    batch = torch.repeat_interleave(torch.arange(nb), torch.tensor(lengths)).to(dev)
    dm.register_batch(batch, ptr, nb, max_nodes=max(lengths), min_nodes=min(lengths))
    pos = torch.rand(N, 2, generator=g).to(dev)
    x = torch.randn(N, F, generator=g).to(dev)
    xx = x.clone().requires_grad_(True)
    gout = torch.randn(N, F, generator=g).to(dev)
    ei = dm.knn_graph(pos, K, batch)
    und = dm.to_undirected(ei, N)
    torch.manual_seed(0)
    pool = dm.EdgePooling(F).to(dev)
    res = {"batch": label, "events": nb, "nodes": N, "edges": int(ei.shape[1]), "min_nodes": min(lengths),
           "max_nodes": max(lengths), "F": F, "k": K, "steps": steps}
    with torch.no_grad():
        score = pool.scores(x, ei, batch)
    grouped = edge_pool._group(ei, N)
    match_only(res, grouped, score, ptr, ei[0], ei[1], N, steps, warmup, dev)

    def edge_pool_step():
        out = pool(xx, ei, batch)[0]
        out.backward(gout[: out.shape[0]])
        xx.grad = None
        pool.zero_grad()

    def graclus_step():
        w = dm.normalized_cut_2d(und, pos)
        cluster = dm.graclus(und, w, N, batch=batch, seed=1)
        out, _pb = dm.max_pool_x(cluster, xx, batch)
        out.backward(gout[: out.shape[0]])
        xx.grad = None

    medians(alternate({"edge_pool_step": edge_pool_step, "graclus_step": graclus_step}, steps, warmup, dev), res)
    res["pooled_rows"] = int(pool(x, ei, batch)[0].shape[0])
    res["launches"].update(edge_pool_step=launches(edge_pool_step, dev), graclus_step=launches(graclus_step, dev))
    res["host_reads"].update(edge_pool_step=host_reads(edge_pool_step, dev), graclus_step=host_reads(graclus_step, dev))
    return res


def run_path(n, steps, warmup, dev):
    """The worst case: one path of n nodes, edge i = (i, i + 1), strictly descending scores."""
    ei = torch.stack([torch.arange(n - 1), torch.arange(1, n)]).to(dev)
    score = torch.arange(n - 1, 0, -1, dtype=torch.float32, device=dev)
    ptr = torch.tensor([0, n], device=dev)
    edges = edge_list_from_edge_index(ei, n, "source_to_target")
    grouped = edge_pool._Grouped(edges, edges.src)
    res = {"batch": f"one path of {n}", "events": 1, "nodes": n, "edges": n - 1, "steps": steps}
    match_only(res, grouped, score, ptr, ei[0], ei[1], n, steps, warmup, dev)
    res["us_per_round"] = round(res["match_native_us"] / max(res["rounds"]["max"], 1), 3)
    res["composed_us_per_round"] = round(res["match_composed_us"] / max(res["rounds"]["composed"], 1), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_pool_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for label, lengths in (("64x4500", [4500] * B), ("ragged 500-8000", ragged_lengths())):
        lines.append(run_batch(label, lengths, a.steps, a.warmup, dev))
        print(json.dumps(lines[-1]), flush=True)
    lines.append(run_path(4500, max(a.steps // 5, 3), min(a.warmup, 2), dev))
    print(json.dumps(lines[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

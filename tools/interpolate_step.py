"""Forward + backward time of knn_interpolate (csrc/interpolate.hip) against the composed torch route, the upstream formula:
knn -> [2, E] sized by a host sync -> index_select -> weights -> two index_add_.

    python tools/interpolate_step.py [--shapes 64x4500] [--ratio 0.25] [--steps 50] [--warmup 10] [--json OUT]

One JSON line per shape: B events of n fine nodes, ceil(ratio n) centres per event from fps, F = 64 features on the
centres, k = 3.  `step_*`: the whole operator, graph build included, native and composed steps alternating inside one
loop, medians of the per-step device time (HIP events).  `aggregate_*`: forward + backward over a prebuilt table and
reverse index (native) or a prebuilt edge index (composed).  `kernels`: the HIP-event brackets of the two native calls,
their compulsory bytes (every distinct row once: x, the table and its distances, out and wsum; for the backward g_out,
wsum, one distance and one position per entry, the reverse index and g_x), the share of the time those bytes take at the
measured copy bandwidth of the part (6.29 TB/s), and `gathered_bytes`, the same with one 4F-byte row per entry (what the
lanes ask of the caches: every x row is read about k Nt / Ns times, every g_out row k times).  `zeros_fill_ms`: what
the zero-filled output allocations of the two wrappers cost over uninitialised ones (out, wsum, g_x), brackets outside
the kernels' own."""
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

F, K, D = 64, 3, 2
COPY_BW = 6.29e12       # bytes / s, float4 copy on an MI355X


def composed(x, pos_x, pos_y, batch_x, batch_y, k, edges=None):
    """torch_geometric.nn.unpool.knn_interpolate as upstream writes it, over this package's knn."""
    with torch.no_grad():
        y_idx, x_idx = dm.knn(pos_x, pos_y, k, batch_x, batch_y) if edges is None else edges
        diff = pos_x.index_select(0, x_idx) - pos_y.index_select(0, y_idx)
        w = 1.0 / torch.clamp((diff * diff).sum(-1, keepdim=True), min=1e-16)
    num = x.new_zeros((pos_y.shape[0], x.shape[1])).index_add_(0, y_idx, x.index_select(0, x_idx) * w)
    den = w.new_zeros((pos_y.shape[0], 1)).index_add_(0, y_idx, w)
    return num / den


def make_inputs(B, n, ratio, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    pos = torch.randn(B * n, D, generator=g).to(dev)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, ptr, B, max_nodes=n, min_nodes=n)
    idx = dm.fps(pos, batch, ratio, random_start=False)
    m = math.ceil(n * ratio)
    assert idx.numel() == B * m
    pos_c, batch_c = pos[idx].contiguous(), batch[idx].contiguous()
    dm.register_batch(batch_c, torch.arange(0, (B + 1) * m, m, dtype=torch.int64, device=dev), B, max_nodes=m, min_nodes=m)
    x = torch.randn(B * m, F, generator=g).to(dev)
    return x, pos_c, pos, batch_c, batch


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


def kernel_bytes(Nt, Ns):
    """{name: (compulsory bytes, bytes with one row per entry)}"""
    E = Nt * K
    fwd = E * 8 + Nt * (4 * F + 4)
    bwd = E * 8 + Nt * 4 + (Ns + 1) * 4 + Ns * 4 * F
    return {"interpolate_fwd": (fwd + Ns * 4 * F, fwd + E * 4 * F),
            "interpolate_bwd": (bwd + Nt * 4 * F, bwd + E * 4 * F)}


def run_shape(B, n, ratio, steps, warmup, dev):
    x, pos_c, pos_f, bc, bf = make_inputs(B, n, ratio, dev)
    Nt, Ns = pos_f.shape[0], pos_c.shape[0]
    g = torch.randn(Nt, F, generator=torch.Generator().manual_seed(2)).to(dev)
    xx = x.clone().requires_grad_(True)

    def step(fn):
        def run():
            fn().backward(g)
            xx.grad = None
        return run

    whole = alternate({"native": step(lambda: dm.knn_interpolate(xx, pos_c, pos_f, bc, bf, k=K)),
                       "composed": step(lambda: composed(xx, pos_c, pos_f, bc, bf, K))}, steps, warmup, dev)

    table = dm.knn_xy_table(pos_c, pos_f, K, bc, bf)
    table.reverse()
    edges = tuple(dm.knn(pos_c, pos_f, K, bc, bf))
    agg = alternate({"native": step(lambda: dm.interpolate_aggregate(xx, table)),
                     "composed": step(lambda: composed(xx, pos_c, pos_f, bc, bf, K, edges))}, steps, warmup, dev)

    # the two native calls on their own brackets (a run of its own: every bracket is two more stream commands)
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, {"interpolate_fwd", "interpolate_bwd"}
    one = step(lambda: dm.interpolate_aggregate(xx, table))
    for _ in range(steps):
        one()
    torch.cuda.synchronize(dev)
    summary = _native.timer.summary()
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()
    kernels = {}
    for name, (nbytes, gathered) in kernel_bytes(Nt, Ns).items():
        ms = summary[name][1]
        kernels[name] = {"mean_ms": round(ms, 4), "bytes": nbytes, "gathered_bytes": gathered,
                         "bound_ms": round(nbytes / COPY_BW * 1e3, 4),
                         "share_of_bound": round(nbytes / COPY_BW * 1e3 / ms, 3) if ms > 0 else None}

    # zero-filled against uninitialised output allocations: out[Nt, F], wsum[Nt], g_x[Ns, F]
    def alloc(make):
        def run():
            make((Nt, F), dtype=torch.float32, device=dev)
            make((Nt,), dtype=torch.float32, device=dev)
            make((Ns, F), dtype=torch.float32, device=dev)
        return run
    fill = alternate({"zeros": alloc(torch.zeros), "empty": alloc(torch.empty)}, steps, warmup, dev)

    def med(v):
        return round(statistics.median(v), 4)
    return {"events": B, "fine": n, "centres": Ns // B, "edges": Nt * K, "F": F, "k": K, "steps": steps,
            "step_native_ms": med(whole["native"]), "step_composed_ms": med(whole["composed"]),
            "step_ratio": round(statistics.median(whole["composed"]) / statistics.median(whole["native"]), 2),
            "aggregate_native_ms": med(agg["native"]), "aggregate_composed_ms": med(agg["composed"]),
            "aggregate_ratio": round(statistics.median(agg["composed"]) / statistics.median(agg["native"]), 2),
            "kernels": kernels, "zeros_fill_ms": round(med(fill["zeros"]) - med(fill["empty"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500"])
    ap.add_argument("--ratio", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interpolate_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes:
        B, n = (int(v) for v in shape.split("x"))
        line = run_shape(B, n, a.ratio, a.steps, a.warmup, dev)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

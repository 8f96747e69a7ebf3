"""Forward + backward time of GravNetConv(64, 64, 4, 22, 16): the fused aggregate (csrc/gravnet.hip) against the composed
route over the same table -- index_select / exp / index_add / scatter_reduce('amax'), the only way to run the layer
without the kernels.

    python tools/gravnet_step.py [--shapes 64x4500 128x1000] [--steps 50] [--warmup 10] [--json OUT]
    rocprofv3 --kernel-trace --stats -d DIR -o gravnet -- python tools/gravnet_step.py --profile --shapes 64x4500

One JSON line per shape.  `layer_*`: the whole layer (four Linears, kNN build in the learned space, aggregate), fused and
composed steps alternating inside one loop, medians of the per-step device time (HIP events).  `aggregate_*`: forward +
backward of the aggregate alone over a prebuilt table and reverse index.  `kernels`: the HIP-event brackets of the two
native calls, their bytes-moved figure (k rows of 4P bytes per target, the table, the outputs; for the backward the same
rows again, the g_out / arg rows walked by source, the reverse index and the 4-byte-per-slot g_d) and the share of the
time those bytes take at the measured copy bandwidth of the part (6.29 TB/s).  --profile runs fused steps only, for a
kernel trace in a process of its own."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native  # noqa: E402

CIN, COUT, S, P, K = 64, 64, 4, 22, 16
COPY_BW = 6.29e12       # bytes / s, float4 copy on an MI355X


def composed_aggregate(h, s, table):
    """The same [mean | max] from torch operators over the table's slots (every row full: events of at least k nodes)."""
    nbr = table.nbr
    N, k = nbr.shape
    src = nbr.reshape(-1).long()
    tgt = torch.arange(N, device=h.device).repeat_interleave(k)
    w = torch.exp(-10.0 * (s.index_select(0, src) - s.index_select(0, tgt)).pow(2).sum(-1))
    msg = h.index_select(0, src) * w.unsqueeze(-1)
    mean = torch.zeros_like(h).index_add(0, tgt, msg) / k
    mx = torch.full_like(h, float("-inf")).scatter_reduce(0, tgt.unsqueeze(-1).expand_as(msg), msg, "amax")
    return torch.cat([mean, mx], 1)


def composed_layer(conv, x, batch):
    s, h = conv.lin_s(x), conv.lin_h(x)
    table = dm.knn_table(s.detach(), conv.k, batch, loop=True)
    return conv.lin_out1(x) + conv.lin_out2(composed_aggregate(h, s, table))


def make_inputs(B, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * n, CIN, generator=g).to(dev)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, ptr, B, max_nodes=n, min_nodes=n)
    return x, batch


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


def kernel_bytes(N):
    E = N * K
    rows = E * 4 * P
    fwd = rows + E * 4 + N * (2 * P * 4 + P + 4) + 2 * N * S * 4
    bwd_t = rows + E * 4 + N * (2 * P * 4 + P + 4) + E * 4 + 2 * N * S * 4
    bwd_s = E * (2 * P * 4 + P) + 2 * E * 4 + N * (P * 4 + 2 * S * 4)
    return {"gravnet_fwd": fwd, "gravnet_bwd": bwd_t + bwd_s}


def run_shape(B, n, steps, warmup, dev, profile):
    x, batch = make_inputs(B, n, dev)
    N = x.shape[0]
    torch.manual_seed(1)
    conv = dm.GravNetConv(CIN, COUT, S, P, K).to(dev)
    g = torch.randn(N, COUT, generator=torch.Generator().manual_seed(2)).to(dev)
    xx = x.clone().requires_grad_(True)

    def layer(fn):
        def step():
            fn(xx, batch).backward(g)
            xx.grad = None
            conv.zero_grad(set_to_none=True)
        return step

    if profile:
        step = layer(conv)
        for _ in range(warmup + steps):
            step()
        torch.cuda.synchronize(dev)
        return None
    lay = alternate({"fused": layer(conv), "composed": layer(lambda a, b: composed_layer(conv, a, b))}, steps, warmup, dev)

    with torch.no_grad():
        s0, h0 = conv.lin_s(x), conv.lin_h(x)
    table = dm.knn_table(s0, K, batch, loop=True)
    table.reverse()
    hh, ss = h0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
    g2 = torch.randn(N, 2 * P, generator=torch.Generator().manual_seed(3)).to(dev)

    def aggregate(fn):
        def step():
            fn(hh, ss, table).backward(g2)
            hh.grad = ss.grad = None
        return step

    agg = alternate({"fused": aggregate(dm.gravnet_aggregate), "composed": aggregate(composed_aggregate)}, steps, warmup, dev)

    # the two native calls on their own brackets (a run of its own: every bracket is two more stream commands)
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, {"gravnet_fwd", "gravnet_bwd"}
    step = aggregate(dm.gravnet_aggregate)
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    summary = _native.timer.summary()
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()
    kernels = {}
    for name, nbytes in kernel_bytes(N).items():
        ms = summary[name][1]
        kernels[name] = {"mean_ms": round(ms, 4), "bytes": nbytes, "bound_ms": round(nbytes / COPY_BW * 1e3, 4),
                         "share_of_bound": round(nbytes / COPY_BW * 1e3 / ms, 3) if ms > 0 else None}

    def med(v):
        return round(statistics.median(v), 4)
    return {"events": B, "nodes": n, "edges": N * K, "S": S, "P": P, "k": K, "steps": steps,
            "layer_fused_ms": med(lay["fused"]), "layer_composed_ms": med(lay["composed"]),
            "layer_ratio": round(statistics.median(lay["composed"]) / statistics.median(lay["fused"]), 2),
            "aggregate_fused_ms": med(agg["fused"]), "aggregate_composed_ms": med(agg["composed"]),
            "aggregate_ratio": round(statistics.median(agg["composed"]) / statistics.median(agg["fused"]), 2),
            "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500", "128x1000"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true", help="fused layer steps only (run under rocprofv3)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gravnet_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes:
        B, n = (int(v) for v in shape.split("x"))
        line = run_shape(B, n, a.steps, a.warmup, dev, a.profile)
        if line is not None:
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""Forward + backward time of the GAT aggregates (csrc/gat.hip) over knn_table(x, 16) at H = 4, C = 16, fp32, against
(a) the composed route over the same table -- index_select of x_l and x_r, leaky_relu, scatter_reduce('amax'), index_add_
for the softmax sum, then the weighted index_add_: what a user would write without the kernels -- and (b)
attention_aggregate (csrc/attention.hip) at the same shape, which gathers two head rows per edge where GAT gathers one.

    python tools/gat_step.py [--shapes 64x4500] [--steps 50] [--warmup 10] [--repeats 5] [--json OUT]
    rocprofv3 --kernel-trace --stats -d DIR -o gat -- python tools/gat_step.py --profile --shapes 64x4500

One JSON line per shape.  The four variants (gat_v2, gat_v1, composed_v2, attention) take turns inside one loop, so drift
of the machine reaches all of them alike; the loop runs `repeats` times.  `*_ms`: the median over the repeats of each
repeat's median per-step device time (HIP events); `*_spread_ms`: the largest minus the smallest repeat median, the
run-to-run spread a difference has to exceed.  `kernels`: the HIP-event brackets of the native calls, the bytes they must
move counting a gathered row once per edge (what the caches serve) and every array once (the least HBM can move), and the
time of the latter at the measured copy bandwidth of the part (6.29 TB/s).  --profile runs fused GAT steps only, for a
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

C, H, K = 16, 4, 16
SLOPE = 0.2
COPY_BW = 6.29e12       # bytes / s, float4 copy on an MI355X


def composed_v2(xl, xr, att, table):
    """GATv2's softmax-weighted sum from torch operators over the table's slots (every row full)."""
    nbr = table.nbr
    N, kk = nbr.shape
    src = nbr.reshape(-1).long()
    tgt = torch.arange(N, device=xl.device).repeat_interleave(kk)
    xj = xl.index_select(0, src)
    score = (torch.nn.functional.leaky_relu(xj + xr.index_select(0, tgt), SLOPE) * att).sum(-1)
    m = torch.full((N, xl.shape[1]), float("-inf"), device=xl.device)
    m = m.scatter_reduce(0, tgt.view(-1, 1).expand_as(score), score.detach(), "amax")
    p = torch.exp(score - m.index_select(0, tgt))
    l = torch.zeros_like(m).index_add_(0, tgt, p)
    alpha = p / l.index_select(0, tgt)
    return torch.zeros_like(xr).index_add_(0, tgt, alpha.unsqueeze(-1) * xj)


def make_inputs(B, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = B * n
    pos = torch.randn(N, 3, generator=g).to(dev)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, ptr, B, max_nodes=n, min_nodes=n)
    t = {name: torch.randn(N, H, C, generator=g).to(dev) for name in ("xl", "xr", "q", "k", "v")}
    t["q"] *= 0.5
    t["k"] *= 0.5
    t["att"] = (torch.randn(H, C, generator=g) / C ** 0.5).to(dev)
    t["s_src"] = torch.randn(N, H, generator=g).to(dev)
    t["s_dst"] = torch.randn(N, H, generator=g).to(dev)
    t["g"] = torch.randn(N, H, C, generator=g).to(dev)
    return t, pos, batch


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def alternate(fns, steps, warmup, dev):
    """{name: [ms]}: the variants take turns inside one loop."""
    ev = {name: [] for name in fns}
    for it in range(warmup + steps):
        for name, fn in fns.items():
            pair = timed(fn)
            if it >= warmup:
                ev[name].append(pair)
    torch.cuda.synchronize(dev)
    return {name: [a.elapsed_time(b) for a, b in pairs] for name, pairs in ev.items()}


def kernel_bytes(N):
    """name -> (bytes with a gathered row counted once per edge, bytes with every array counted once)."""
    E = N * K
    row = H * C * 4
    sc = H * 4          # one scalar per (node or edge, head)
    ids = E * 4
    work = 2 * E * sc   # alpha and g_score, written once and read once
    v2_fwd = 2 * E * row + ids + N * (2 * row + sc) + row                      # x_l for the score and for the sum; x_r, out, lse
    rev = ids + N * 4   # the by-source index: rev_pos and rev_ptr
    v2_bwd = E * row + ids + N * (5 * row + sc) + work + 2 * E * row + rev + work + N * 2 * row
    v1_fwd = E * row + E * sc + ids + N * (row + 2 * sc)
    v1_bwd = E * row + E * sc + ids + N * (2 * row + 3 * sc) + work + E * row + rev + work + N * (row + sc)
    at_fwd = 2 * E * row + ids + N * (2 * row + sc)
    at_bwd = 2 * E * row + ids + N * (4 * row + sc) + work + 2 * E * row + rev + work + N * 2 * row
    once = {
        "gat_v2_fwd": N * (3 * row + sc) + ids,
        "gat_v2_bwd": N * (8 * row + sc) + ids + rev + 2 * work,             # x_l, x_r, out, g_out, g_x_r, g_att rows | g_x_l
        "gat_v1_fwd": N * (2 * row + 3 * sc) + ids,
        "gat_v1_bwd": N * (4 * row + 5 * sc) + ids + rev + 2 * work,
        "attention_fwd": N * (4 * row + sc) + ids,
        "attention_bwd": N * (10 * row + sc) + ids + rev + 2 * work,
    }
    moved = {"gat_v2_fwd": v2_fwd, "gat_v2_bwd": v2_bwd, "gat_v1_fwd": v1_fwd, "gat_v1_bwd": v1_bwd,
             "attention_fwd": at_fwd, "attention_bwd": at_bwd}
    return {name: (moved[name], once[name]) for name in moved}


def bracket(step, names, steps, dev):
    """Mean ms of the native calls `names` over `steps` runs of `step`, each call on its own HIP-event bracket."""
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, set(names)
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    summary = _native.timer.summary()
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()
    return {name: summary[name][1] for name in names}


def run_shape(B, n, steps, warmup, repeats, dev, profile):
    t, pos, batch = make_inputs(B, n, dev)
    N = B * n
    table = dm.knn_table(pos, K, batch, loop=True)
    table.reverse()
    assert bool((table.nbr >= 0).all())
    leaves = {name: t[name].clone().requires_grad_(True) for name in ("xl", "xr", "att", "s_src", "s_dst", "q", "k", "v")}

    def stepper(fn, *names):
        args = [leaves[name] for name in names]

        def step():
            fn(*args, table).backward(t["g"])
            for a in args:
                a.grad = None
        return step

    fns = {
        "gat_v2": stepper(lambda xl, xr, att, tb: dm.gat_aggregate(xl, xr, att, tb, SLOPE), "xl", "xr", "att"),
        "gat_v1": stepper(lambda xl, ss, sd, tb: dm.gat_v1_aggregate(xl, ss, sd, tb, SLOPE), "xl", "s_src", "s_dst"),
        "composed_v2": stepper(composed_v2, "xl", "xr", "att"),
        "attention": stepper(dm.attention_aggregate, "q", "k", "v"),
    }
    if profile:
        for _ in range(warmup + steps):
            fns["gat_v2"]()
            fns["gat_v1"]()
        torch.cuda.synchronize(dev)
        return None

    # the fused v2 result is the composed one (inside the bars of the tests) at the size that is timed
    with torch.no_grad():
        a = dm.gat_aggregate(t["xl"], t["xr"], t["att"], table, SLOPE)
        b = composed_v2(t["xl"], t["xr"], t["att"], table)
        max_diff = float((a - b).abs().max())

    meds = {name: [] for name in fns}
    for r in range(repeats):
        res = alternate(fns, steps, warmup if r == 0 else 2, dev)
        for name, v in res.items():
            meds[name].append(statistics.median(v))
    line = {"events": B, "nodes": n, "edges": N * K, "H": H, "C": C, "k": K, "steps": steps, "repeats": repeats,
            "fused_vs_composed_max_abs_diff": max_diff}
    for name, v in meds.items():
        line[name + "_ms"] = round(statistics.median(v), 4)
        line[name + "_spread_ms"] = round(max(v) - min(v), 4)
    line["composed_over_gat_v2"] = round(line["composed_v2_ms"] / line["gat_v2_ms"], 2)
    line["attention_over_gat_v2"] = round(line["attention_ms"] / line["gat_v2_ms"], 3)

    ms = {}
    for mode, step in (("gat_v2", fns["gat_v2"]), ("gat_v1", fns["gat_v1"])):
        got = bracket(step, ("gat_fwd", "gat_bwd"), steps, dev)
        ms[mode + "_fwd"], ms[mode + "_bwd"] = got["gat_fwd"], got["gat_bwd"]
    ms.update(bracket(fns["attention"], ("attention_fwd", "attention_bwd"), steps, dev))
    kernels = {}
    for name, (nbytes, once) in kernel_bytes(N).items():
        kernels[name] = {"mean_ms": round(ms[name], 4), "bytes": nbytes, "bytes_per_edge": round(nbytes / (N * K), 1),
                         "once_bytes": once, "once_bound_ms": round(once / COPY_BW * 1e3, 4)}
    line["kernels"] = kernels
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="fused GAT steps only (run under rocprofv3)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes:
        B, n = (int(v) for v in shape.split("x"))
        line = run_shape(B, n, a.steps, a.warmup, a.repeats, dev, a.profile)
        if line is not None:
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

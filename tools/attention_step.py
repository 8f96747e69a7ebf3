"""Forward + backward time of TransformerConv(64, 16, heads=4) over knn_table(x, 16): the fused aggregate
(csrc/attention.hip) against the composed route over the same table -- index_select of q / k / v, scatter_reduce('amax'),
index_add_ for the softmax sum, then the weighted index_add_: what a user would write without the kernels.

    python tools/attention_step.py [--shapes 64x4500 128x1000] [--steps 50] [--warmup 10] [--json OUT]
    rocprofv3 --kernel-trace --stats -d DIR -o attention -- python tools/attention_step.py --profile --shapes 64x4500

One JSON line per shape.  `layer_*`: the whole layer (four Linears, aggregate) over a prebuilt table, fused and composed
steps alternating inside one loop, medians of the per-step device time (HIP events).  `aggregate_*`: forward + backward
of the aggregate alone.  `kernels`: the HIP-event brackets of the two native calls, the bytes they must move (per edge a
k and a v head row of 4C bytes per head and the table entry, per node the q / out / lse rows; for the backward the k and v
rows again, the g_out and q rows walked by source, the reverse index and the two 4-byte-per-(edge, head) work arrays,
written once and read once) and the share of the time those bytes take at the measured copy bandwidth of the part
(6.29 TB/s).  `bytes` counts a gathered row once per edge, so it is what the caches serve, not what HBM must: a share
above 1 says the gathers hit the L2 / Infinity Cache.  `once_bytes` is every array the call touches counted once -- the
least HBM can move -- and `once_bound_ms` its time at the same rate.  --profile runs fused aggregate steps only, for a
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

CIN, C, H, K = 64, 16, 4, 16
COPY_BW = 6.29e12       # bytes / s, float4 copy on an MI355X


def composed_aggregate(q, k, v, table):
    """The same softmax-weighted sum from torch operators over the table's slots (every row full)."""
    nbr = table.nbr
    N, kk = nbr.shape
    src = nbr.reshape(-1).long()
    tgt = torch.arange(N, device=q.device).repeat_interleave(kk)
    score = (q.index_select(0, tgt) * k.index_select(0, src)).sum(-1) / (q.shape[2] ** 0.5)
    m = torch.full((N, q.shape[1]), float("-inf"), device=q.device)
    m = m.scatter_reduce(0, tgt.view(-1, 1).expand_as(score), score.detach(), "amax")
    p = torch.exp(score - m.index_select(0, tgt))
    l = torch.zeros_like(m).index_add_(0, tgt, p)
    alpha = p / l.index_select(0, tgt)
    return torch.zeros_like(q).index_add_(0, tgt, alpha.unsqueeze(-1) * v.index_select(0, src))


def layer(conv, x, table, aggregate):
    q = conv.lin_query(x).view(-1, H, C)
    k = conv.lin_key(x).view(-1, H, C)
    v = conv.lin_value(x).view(-1, H, C)
    return aggregate(q, k, v, table).reshape(-1, H * C) + conv.lin_skip(x)


def make_inputs(B, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * n, CIN, generator=g).to(dev)
    pos = torch.randn(B * n, 3, generator=g).to(dev)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, ptr, B, max_nodes=n, min_nodes=n)
    return x, pos, batch


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
    row = H * C * 4
    fwd = 2 * E * row + E * 4 + N * (2 * row + H * 4)
    bwd_t = 2 * E * row + E * 4 + N * (4 * row + H * 4) + 2 * E * H * 4
    bwd_s = 2 * E * row + 2 * E * 4 + 2 * E * H * 4 + N * 2 * row
    # every array once: q, k, v, out (+ g_out, g_q | g_out, q, g_k, g_v) rows, lse, the ids / reverse index, the work arrays
    once_fwd = N * (4 * row + H * 4) + E * 4
    once_bwd = N * (6 * row + H * 4) + E * 4 + 2 * E * H * 4 + N * 4 * row + E * 4 + N * 4 + 2 * E * H * 4
    return {"attention_fwd": (fwd, once_fwd), "attention_bwd": (bwd_t + bwd_s, once_bwd)}


def run_shape(B, n, steps, warmup, dev, profile):
    x, pos, batch = make_inputs(B, n, dev)
    N = x.shape[0]
    torch.manual_seed(1)
    conv = dm.TransformerConv(CIN, C, heads=H).to(dev)
    table = dm.knn_table(pos, K, batch, loop=True)
    table.reverse()
    with torch.no_grad():
        q0, k0, v0 = (lin(x).view(-1, H, C) for lin in (conv.lin_query, conv.lin_key, conv.lin_value))
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    g2 = torch.randn(N, H, C, generator=torch.Generator().manual_seed(3)).to(dev)

    def aggregate(fn):
        def step():
            fn(qq, kk, vv, table).backward(g2)
            qq.grad = kk.grad = vv.grad = None
        return step

    if profile:
        step = aggregate(dm.attention_aggregate)
        for _ in range(warmup + steps):
            step()
        torch.cuda.synchronize(dev)
        return None

    g = torch.randn(N, H * C, generator=torch.Generator().manual_seed(2)).to(dev)
    xx = x.clone().requires_grad_(True)

    def layer_step(fn):
        def step():
            layer(conv, xx, table, fn).backward(g)
            xx.grad = None
            conv.zero_grad(set_to_none=True)
        return step

    lay = alternate({"fused": layer_step(dm.attention_aggregate), "composed": layer_step(composed_aggregate)}, steps, warmup,
                    dev)
    agg = alternate({"fused": aggregate(dm.attention_aggregate), "composed": aggregate(composed_aggregate)}, steps, warmup, dev)

    # the two native calls on their own brackets (a run of its own: every bracket is two more stream commands)
    _native.timer.calibrate(dev)
    _native.timer.reset()
    _native.timer.enabled, _native.timer.only = True, {"attention_fwd", "attention_bwd"}
    step = aggregate(dm.attention_aggregate)
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    summary = _native.timer.summary()
    _native.timer.enabled, _native.timer.only = False, None
    _native.timer.reset()
    kernels = {}
    for name, (nbytes, once) in kernel_bytes(N).items():
        ms = summary[name][1]
        kernels[name] = {"mean_ms": round(ms, 4), "bytes": nbytes, "bound_ms": round(nbytes / COPY_BW * 1e3, 4),
                         "share_of_bound": round(nbytes / COPY_BW * 1e3 / ms, 3) if ms > 0 else None,
                         "once_bytes": once, "once_bound_ms": round(once / COPY_BW * 1e3, 4)}

    def med(v):
        return round(statistics.median(v), 4)
    return {"events": B, "nodes": n, "edges": N * K, "H": H, "C": C, "k": K, "steps": steps,
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
    ap.add_argument("--profile", action="store_true", help="fused aggregate steps only (run under rocprofv3)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_step.py measures on a GPU; none is visible")
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

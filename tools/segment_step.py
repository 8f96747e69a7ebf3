"""Forward + backward time of the segment reductions of csrc/segment.hip against the composition a user would write from
torch's own operators (scatter_reduce / index_add_ plus autograd) on the same device:

    rows     288 000 rows x 16 entries x H = 64 (the edges of a kNN graph), each reduction twice: scatter_softmax /
             scatter_mean / scatter_min with the int64 index, as a user calls them (they group the index on every call:
             an int32 cast, the reverse-index sort, the range and grouping checks and their one host sync), and the
             kernel pair alone through softmax(src, ptr=ptr) / segment_csr(src, ptr), which need no grouping
    outlier  the same rows plus one row of 2 000 entries, through scatter_softmax: the longest row picks the form for
             the whole call, so every 16-entry row gets a workgroup; beside it the wavefront form of the same call
    events   softmax(src, ptr=ptr) over 64 events x 4500 nodes at H = 1 and H = 32 (an attention read-out over events)

    python tools/segment_step.py [--steps 300] [--warmup 20] [--json OUT]
    rocprofv3 --kernel-trace --stats -d DIR -o segment -- python tools/segment_step.py --profile

One JSON line per case.  The versions take turns inside one loop, so drift of the machine reaches all alike; the event
cases also time the wavefront form of the same kernels (hint 0), the form a workgroup per row is there to beat.
`*_ms`: the median per-step time of forward + backward between two HIP events (a host sync inside a step, as the
grouping of an index makes, is inside the bracket); `scatter_ms` the torch_scatter-style call with the index, `kernels_ms`
the ptr / segment_csr call, `composed_ms` the composition from torch operators (given the index); `bytes`: what the kernel pair must move,
every array once, computed from the shapes; `floor_ms`: that traffic at the measured copy bandwidth of the part
(6.29 TB/s).  --profile runs the kernels only, for a kernel trace in a process of its own."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd.scatter import _SegmentSoftmaxRows  # noqa: E402

COPY_BW = 6.29e12       # bytes / s, float4 copy on an MI355X


def composed_softmax(src, ids, n):
    idx = ids.view(-1, 1).expand_as(src)
    m = torch.full((n, src.shape[1]), float("-inf"), device=src.device).scatter_reduce(0, idx, src.detach(), "amax")
    p = torch.exp(src - m.index_select(0, ids))
    l = torch.zeros_like(m).index_add_(0, ids, p)
    return p / l.index_select(0, ids)


def composed_mean(src, ids, n, cnt):
    return torch.zeros((n, src.shape[1]), device=src.device).index_add_(0, ids, src) / cnt


def composed_min(src, ids, n):
    return torch.zeros((n, src.shape[1]), device=src.device).scatter_reduce(0, ids.view(-1, 1).expand_as(src), src, "amin",
                                                                           include_self=False)


def step(fn, src, g):
    src.grad = None
    fn(src).backward(g)


def alternate(fns, steps, warmup):
    ev = {name: [] for name in fns}
    for it in range(warmup + steps):
        for name, fn in fns.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if it >= warmup:
                ev[name].append((a, b))
    torch.cuda.synchronize()
    return {name: statistics.median(a.elapsed_time(b) for a, b in pairs) for name, pairs in ev.items()}


def cases(dev):
    g = torch.Generator().manual_seed(0)
    n, k, H = 288000, 16, 64
    ids = torch.repeat_interleave(torch.arange(n, device=dev), k)
    ptr = torch.arange(0, (n + 1) * k, k, dtype=torch.int64, device=dev)
    src = (torch.randn(n * k, H, generator=g) * 5).to(dev).requires_grad_(True)
    ge = torch.randn(n * k, H, generator=g).to(dev)
    gr = torch.randn(n, H, generator=g).to(dev)
    cnt = torch.full((n, 1), float(k), device=dev)
    E4 = n * k * H * 4
    R4 = n * H * 4
    # softmax: fwd reads src, writes y (+ lse); bwd reads y and g, writes g_src.  mean / min: fwd reads src, writes out
    # (+ arg); bwd reads g_out (+ arg), writes g_src.
    yield ("softmax rows", src, ge, lambda s: dm.softmax(s, ptr=ptr), lambda s: composed_softmax(s, ids, n),
           5 * E4 + R4, {"scatter": lambda s: dm.scatter_softmax(s, ids, dim=0, dim_size=n)})
    yield ("mean rows", src, gr, lambda s: dm.segment_csr(s, ptr, reduce="mean"),
           lambda s: composed_mean(s, ids, n, cnt), 2 * E4 + 2 * R4,
           {"scatter": lambda s: dm.scatter_mean(s, ids, dim=0, dim_size=n)})
    yield ("min rows", src, gr, lambda s: dm.segment_csr(s, ptr, reduce="min"), lambda s: composed_min(s, ids, n),
           2 * E4 + 4 * R4, {"scatter": lambda s: dm.scatter_min(s, ids, dim=0, dim_size=n)[0]})
    del src, ge
    long_row = 2000
    ids2 = torch.cat([ids, torch.full((long_row,), n, device=dev)])
    rp2 = torch.cat([ptr, ptr[-1:] + long_row]).to(torch.int32)
    src2 = (torch.randn(n * k + long_row, H, generator=g) * 5).to(dev).requires_grad_(True)
    ge2 = torch.randn(n * k + long_row, H, generator=g).to(dev)
    yield ("softmax rows + one row of 2000", src2, ge2, lambda s: dm.scatter_softmax(s, ids2, dim=0, dim_size=n + 1),
           lambda s: composed_softmax(s, ids2, n + 1), 5 * (E4 + long_row * H * 4) + R4,
           {"wavefront_form": lambda s: _SegmentSoftmaxRows.apply(s, rp2, False, 0)})
    del src2, ge2
    B, nodes = 64, 4500
    eptr = torch.arange(0, (B + 1) * nodes, nodes, dtype=torch.int64, device=dev)
    eids = torch.repeat_interleave(torch.arange(B, device=dev), nodes)
    for H in (1, 32):
        s = (torch.randn(B * nodes, H, generator=g) * 5).to(dev).requires_grad_(True)
        ge = torch.randn(B * nodes, H, generator=g).to(dev)
        rp = eptr.to(torch.int32)
        yield (f"softmax events H={H}", s, ge, lambda t: dm.softmax(t, ptr=eptr), lambda t: composed_softmax(t, eids, B),
               5 * B * nodes * H * 4 + B * H * 4,
               {"wavefront_form": lambda t, rp=rp: _SegmentSoftmaxRows.apply(t, rp, False, 0)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile", action="store_true", help="the kernels only, 20 steps per case")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for name, src, g, ours, composed, nbytes, others in cases(dev):
        if args.profile:
            for _ in range(20):
                step(ours, src, g)
            torch.cuda.synchronize()
            continue
        fns = {"kernels": lambda: step(ours, src, g), "composed": lambda: step(composed, src, g)}
        for other, fn in others.items():
            fns[other] = lambda fn=fn: step(fn, src, g)
        ms = alternate(fns, args.steps, args.warmup)
        line = {"case": name, **{f"{k}_ms": round(v, 4) for k, v in ms.items()}, "bytes": nbytes,
                "floor_ms": round(nbytes / COPY_BW * 1e3, 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()

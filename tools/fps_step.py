"""Time of farthest point sampling: the kernel (csrc/fps.hip, one launch for all events and all picks) against the same
greedy loop written in batched torch operators over the equal-size events -- one pass of gather / subtract / square /
sum / minimum / argmax per pick, no host read inside the loop.  There is no other way to run fps without the kernel.

    python tools/fps_step.py [--shapes 64x4500 128x1000] [--dims 2 32] [--ratios 0.25 0.5] [--steps 10] [--warmup 2] [--json OUT]

One JSON line per (shape, D, ratio): medians of the device time between HIP events.  `fps_ms`: dmet_fps_f32 alone (out_ptr
prebuilt, start at node 0); `us_per_pick`: that time over the m - 1 picks after the start; `torch_loop_ms`: the torch loop;
`ratio`: torch_loop_ms / fps_ms; `same_ids`: the share of ids the two agree on (the torch loop sums squares without the
contract's fma chain and its argmax promises no tie order, so it is a timing baseline, not a reference).  The two take
turns inside one loop, so drift of the machine reaches both alike."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deepmetv2_amd import _native  # noqa: E402


def torch_loop(x3, m):
    """[B, m] event-local ids of the greedy loop over x3[B, n, D], start at node 0 of every event."""
    B, n, _D = x3.shape
    rows = torch.arange(B, device=x3.device)
    s = torch.zeros(B, dtype=torch.int64, device=x3.device)
    dist = torch.full((B, n), float("inf"), device=x3.device)
    out = torch.empty((B, m), dtype=torch.int64, device=x3.device)
    for i in range(m):
        out[:, i] = s
        if i + 1 == m:
            break
        d = (x3 - x3[rows, s].unsqueeze(1)).pow(2).sum(-1)
        dist = torch.minimum(dist, d)
        s = dist.argmax(1)
    return out


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return a, b, out


def run(B, n, D, ratio, steps, warmup, dev):
    x = torch.randn(B * n, D, generator=torch.Generator().manual_seed(B + n + D)).to(dev)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    m = int(torch.ceil(torch.tensor(float(n)) * torch.tensor(ratio)).item())
    out_ptr = torch.arange(0, (B + 1) * m, m, dtype=torch.int64, device=dev)
    x3 = x.view(B, n, D)
    lo = ptr[:-1].view(B, 1)
    fns = {"fps": lambda: _native.fps(x, ptr, out_ptr, None, B * m), "torch": lambda: torch_loop(x3, m)}
    ev = {k: [] for k in fns}
    last = {}
    for it in range(warmup + steps):
        for k, fn in fns.items():
            a, b, out = timed(fn)
            last[k] = out
            if it >= warmup:
                ev[k].append((a, b))
    torch.cuda.synchronize(dev)
    ms = {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
    same = float((last["fps"].view(B, m) == last["torch"] + lo).float().mean())
    return {"events": B, "nodes": n, "D": D, "ratio": ratio, "m": m, "steps": steps, "fps_ms": round(ms["fps"], 4),
            "us_per_pick": round(ms["fps"] * 1e3 / max(m - 1, 1), 3), "torch_loop_ms": round(ms["torch"], 3),
            "torch_us_per_pick": round(ms["torch"] * 1e3 / max(m - 1, 1), 2),
            "ratio_torch_over_fps": round(ms["torch"] / ms["fps"], 1), "same_ids": round(same, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500", "128x1000"])
    ap.add_argument("--dims", nargs="+", type=int, default=[2, 32])
    ap.add_argument("--ratios", nargs="+", type=float, default=[0.25, 0.5])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes:
        B, n = (int(v) for v in shape.split("x"))
        for D in a.dims:
            for ratio in a.ratios:
                line = run(B, n, D, ratio, a.steps, a.warmup, dev)
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

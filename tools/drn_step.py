"""DynamicReductionNetwork forward + backward rate, with a per-operator breakdown and the graclus round statistics.

    python tools/drn_step.py [--shapes 64x4500 128x1000] [--hidden 64] [--k 16] [--steps 10] [--warmup 3] [--autocast]
                             [--autocast-dtype {bfloat16,float16}] [--json OUT]

Measurement only (bench.py measures the flagship model).  The rate is taken over `--steps` back-to-back forward +
backward passes (no optimizer).  The breakdown is a separate pass that synchronises after every stage, so its stages are
device time plus the host time the stage itself spends (one host sync each in to_undirected, knn_graph with loop=False,
and max_pool_x).  --autocast runs every pass under torch.autocast("cuda", dtype=torch.bfloat16): the EdgeConvs then take
the bf16 matrix-core route (csrc/edgemlp_bf16.hip); with --autocast-dtype float16 under torch.autocast("cuda",
dtype=torch.float16), the fp16 one (the same kernels on the fp16 matrix cores)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native, pool  # noqa: E402


def make_batch(B, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B * n, 5, generator=g).to(dev)
    ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    dm.register_batch(batch, ptr, B, max_nodes=n, min_nodes=n)
    class D:  # noqa: E306
        pass
    d = D()
    d.x, d.batch = x, batch
    return d


def breakdown(m, data):
    """Seconds per stage of one forward (synchronised after each) + graclus rounds per event."""
    t = {}
    rounds = []

    def stage(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t[name] = t.get(name, 0.0) + time.perf_counter() - t0
        return r

    x = stage("inputnet", lambda: m.inputnet(m.datanorm * data.x))
    batch = data.batch
    for i, conv in enumerate((m.edgeconv1, m.edgeconv2), 1):
        N = x.shape[0]
        knn = stage(f"knn_graph{i}", lambda: dm.knn_graph(x, m.k, batch, loop=False, flow=conv.flow))
        ei = stage(f"to_undirected{i}", lambda: dm.to_undirected(knn, num_nodes=N))
        x = stage(f"edgeconv{i}", lambda: conv(x, ei))
        w = stage(f"normalized_cut{i}", lambda: dm.normalized_cut_2d(ei, x))
        cl = stage(f"graclus{i}", lambda: dm.graclus(ei, w, N, batch=batch, seed=i))
        # the same matching again with the round counter on (statistics only; not part of the timed stages)
        rowptr, col, ww = pool._csr(ei, N, w)
        ptr = dm.graph.batch_info(batch, N, x.device).ptr
        _c, _p, r = _native.graclus(rowptr, col, ww, ptr, i, want_rounds=True)
        rounds.append(r.cpu())
        x, batch = stage(f"max_pool_x{i}", lambda: dm.max_pool_x(cl, x, batch))
    out = stage("global_pool+output", lambda: m.output(dm.global_max_pool(x, batch)).squeeze(-1))
    stage("backward", lambda: out.float().sum().backward())
    return t, rounds


def run(B, n, hidden, k, steps, warmup, dev, autocast=False, autocast_dtype=torch.bfloat16):
    torch.manual_seed(0)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=hidden, k=k).to(dev).train()
    data = make_batch(B, n, dev)
    with torch.autocast("cuda", dtype=autocast_dtype, enabled=autocast):
        for _ in range(warmup):
            m(data).float().sum().backward()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            m(data).float().sum().backward()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        t, rounds = breakdown(m, data)
    res = {"shape": f"{B}x{n}", "hidden": hidden, "k": k, "autocast": autocast, "ms_per_step": dt * 1e3,
           "events_per_s": B / dt, "breakdown_ms": {kk: v * 1e3 for kk, v in t.items()}}
    for i, r in enumerate(rounds, 1):
        res[f"graclus{i}_rounds_mean"] = float(r.float().mean())
        res[f"graclus{i}_rounds_max"] = int(r.max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4500", "128x1000"])
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--autocast", action="store_true", help="autocast (the EdgeConvs' 16-bit matrix-core route)")
    ap.add_argument("--autocast-dtype", choices=("bfloat16", "float16"), default="bfloat16",
                    help="autocast dtype with --autocast (default bfloat16)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    for s in a.shapes:
        B, n = (int(v) for v in s.split("x"))
        r = run(B, n, a.hidden, a.k, a.steps, a.warmup, dev, a.autocast, getattr(torch, a.autocast_dtype))
        if a.autocast:
            r["autocast_dtype"] = a.autocast_dtype
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

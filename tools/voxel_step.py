"""Time of `voxel_grid` (csrc/voxel.hip) against the same formula composed from torch operators, of
`max_pool_x(voxel_grid(...), x, batch)` forward + backward on the registered result (one ranking per event,
dmet_voxel_coarsen) against the same ids as a clone (the generic branch: a global stable sort, cumsum, scatters,
searchsorted), and of the coarsening alone against its traffic floor.

    python tools/voxel_step.py [--steps 200] [--warmup 20] [--json OUT]

Two batches of the same total, D = 2 as (eta, phi) uniform on [-2.5, 2.5] x [-pi, pi], F = 64 fp32: 64 events of 4500
nodes, and 64 events of 500 to 8000 nodes (seeded, adjusted to the same 288 000).  The cell size puts about 4 nodes of a
4500-node event into a cell.  One JSON line per batch.  The variants take turns inside one loop; medians of the per-step
device time (HIP events; a pooling step reads three numbers from the device and includes that wait).  `launches`: the
device kernels of one step, counted by torch.profiler.  `coarsen_us`: HIP-event bracket of dmet_voxel_coarsen's two
launches in a run of their own; `coarsen_floor_us`: 4 N bytes read and 16 N + 12 C written at 6.3 TB/s.  `equal`: the
ids and the pooled rows of the variants agree bit for bit at the timed size."""
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
from deepmetv2_amd.graph import _registry_get  # noqa: E402
from deepmetv2_amd.pool import _voxel_registry  # noqa: E402

F, B, TOTAL = 64, 64, 64 * 4500
LO, HI = (-2.5, -math.pi), (2.5, math.pi)
SIZE = tuple(math.sqrt((HI[0] - LO[0]) * (HI[1] - LO[1]) * 4 / 4500) for _ in range(2))    # 4 nodes a cell at n = 4500
HBM_BYTES_PER_US = 6.3e6


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


def composed_voxel_grid(pos, size, batch, start, end, nb):
    """PyG's voxel_grid as torch_cluster's formula in torch operators (no clamp: the positions lie inside the grid)."""
    p = torch.cat([pos, batch.view(-1, 1).to(pos.dtype)], 1)
    size = torch.cat([size, size.new_ones(1)])
    start = torch.cat([start, start.new_zeros(1)])
    end = torch.cat([end, end.new_full((1,), nb - 1)])
    nvox = ((end - start) / size).trunc().to(torch.int64) + 1
    mul = torch.cat([nvox.new_ones(1), nvox.cumprod(0)[:-1]])
    return (((p - start) / size).trunc().to(torch.int64) * mul).sum(1)


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
    """{kernel: us per call}: HIP-event brackets of the native calls, in a run of their own."""
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


def launches(fn, dev):
    """Device kernels of one call, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize(dev)
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name)
    except Exception:       # noqa: BLE001 -- a figure for the table, not a result
        return None


def run_batch(label, lengths, steps, warmup, dev):
    g = torch.Generator().manual_seed(1)
    N, nb = sum(lengths), len(lengths)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(lengths).cumsum(0)]).to(dev)
    batch = torch.repeat_interleave(torch.arange(nb), torch.tensor(lengths)).to(dev)
    dm.register_batch(batch, ptr, nb, max_nodes=max(lengths), min_nodes=min(lengths))
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    pos = (lo + (hi - lo) * torch.rand(N, 2, generator=g)).to(dev)
    x = torch.randn(N, F, generator=g).to(dev)
    xx = x.clone().requires_grad_(True)
    gout = torch.randn(N, F, generator=g).to(dev)
    size_d, lo_d, hi_d = torch.tensor(SIZE, device=dev), lo.to(dev), hi.to(dev)

    def pool_step(clone):
        def run():
            cluster = dm.voxel_grid(pos, SIZE, batch, LO, HI)
            out, _pb = dm.max_pool_x(cluster.clone() if clone else cluster, xx, batch)
            out.backward(gout[: out.shape[0]])
            xx.grad = None
        return run

    res = {"batch": label, "events": nb, "nodes": N, "min_nodes": min(lengths), "max_nodes": max(lengths), "F": F,
           "size": [round(s, 5) for s in SIZE], "steps": steps}
    with torch.no_grad():
        ids = dm.voxel_grid(pos, SIZE, batch, LO, HI)
        res["ids_equal"] = bool(torch.equal(ids, composed_voxel_grid(pos, size_d, batch, lo_d, hi_d, nb)))
        a, pa = dm.max_pool_x(ids, x, batch)
        b, pb = dm.max_pool_x(ids.clone(), x, batch)
        res["pool_equal"] = bool(torch.equal(a, b)) and bool(torch.equal(pa, pb))
        res["clusters"] = int(a.shape[0])
    rec = _registry_get(_voxel_registry, ids)
    t = alternate({"voxel_grid_native": lambda: dm.voxel_grid(pos, SIZE, batch, LO, HI),
                   "voxel_grid_composed": lambda: composed_voxel_grid(pos, size_d, batch, lo_d, hi_d, nb),
                   "pool_registered": pool_step(False), "pool_clone": pool_step(True)}, steps, warmup, dev)
    res["launches"] = {"pool_registered": launches(pool_step(False), dev), "pool_clone": launches(pool_step(True), dev),
                       "voxel_grid_native": launches(lambda: dm.voxel_grid(pos, SIZE, batch, LO, HI), dev),
                       "voxel_grid_composed": launches(lambda: composed_voxel_grid(pos, size_d, batch, lo_d, hi_d, nb), dev)}
    k = bracket(("voxel_coarsen", "voxel_cells"), lambda: (dm.voxel_grid(pos, SIZE, batch, LO, HI),
                                                           _native._voxel_coarsen(rec.cell, rec.ptr)), steps, dev)
    res["coarsen_us"], res["cells_us"] = k.get("voxel_coarsen"), k.get("voxel_cells")
    res["coarsen_bytes"] = 4 * N + 16 * N + 12 * res["clusters"]
    res["coarsen_floor_us"] = round(res["coarsen_bytes"] / HBM_BYTES_PER_US, 2)
    for name, v in t.items():
        q = statistics.quantiles(v, n=4)
        res[name + "_us"] = round(statistics.median(v) * 1e3, 2)
        res[name + "_quartiles_us"] = [round(q[0] * 1e3, 2), round(q[2] * 1e3, 2)]
    res["voxel_grid_ratio"] = round(res["voxel_grid_composed_us"] / res["voxel_grid_native_us"], 2)
    res["pool_ratio"] = round(res["pool_clone_us"] / res["pool_registered_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_step.py measures on a GPU; none is visible")
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

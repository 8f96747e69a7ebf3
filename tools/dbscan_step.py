"""Time of `dbscan` over (eta, phi) with periodic phi and of its parts: the radius_table build, the components kernel
(csrc/components.hip) in connected-components mode and in DBSCAN mode on that table, and the whole call.

    python tools/dbscan_step.py [--steps 50] [--warmup 10] [--repeats 5] [--json OUT] [--no-host]

Two batches of seeded synthetic events (deepmetv2_amd.synth: eta uniform in [-5, 5], phi in [-pi, pi]): 64 events of
4500 nodes and 128 of 1000.  eps is chosen from the point density so that a neighbourhood holds 5.5 points on average,
itself included, and min_samples = 5: core points, border points and noise all occur (their shares are in the line).
Every part is timed by HIP events around the call, `steps` calls after `warmup`, the median of them; that is repeated
`repeats` times: `*_us` is the median of the medians, `*_spread_us` their largest minus their smallest.  The parts are
timed in loops of their own, not in turns.

`floor_us`: the bytes the kernel cannot avoid -- the valid table entries and the counts read once (4 bytes each), the
labels written (8 per node; DBSCAN mode: the core byte and the per-event count too) -- at the measured copy bandwidth of
the part (6.29 TB/s); `*_floor_share` = floor / measured.
For orientation only, on the host with 16 threads: scipy's connected_components on the same entries as one sparse
matrix, and sklearn's DBSCAN(metric='precomputed') event by event on the same entries (`host_*_ms`; the matrices are
built outside the timed region; one run each, no spread)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native, synth  # noqa: E402

HBM_BYTES_PER_US = 6.29e6
MIN_SAMPLES, MAX_NBR, MEAN_HITS = 5, 64, 5.5
PERIOD = [None, 2 * math.pi]


def measure(fn, steps, warmup, repeats, dev):
    """(median of the repeats' medians, their spread) in us."""
    meds = []
    for _ in range(repeats):
        pairs = []
        for it in range(warmup + steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if it >= warmup:
                pairs.append((a, b))
        torch.cuda.synchronize(dev)
        meds.append(statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3)
    return round(statistics.median(meds), 2), round(max(meds) - min(meds), 2)


def host_reference(nbr, cnt, ptr, res):
    import numpy as np
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from sklearn.cluster import DBSCAN
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        threadpool_limits = None
    nbr, cnt, ptr = nbr.cpu().numpy(), cnt.cpu().numpy(), ptr.cpu().numpy()
    N, k = nbr.shape
    valid = np.arange(k)[None, :] < cnt[:, None]
    tgt = np.repeat(np.arange(N), cnt)
    src = nbr[valid]
    whole = sp.coo_matrix((np.ones(len(src)), (tgt, src)), shape=(N, N)).tocsr()
    t0 = time.perf_counter()
    connected_components(whole, directed=True, connection="weak")
    res["host_scipy_cc_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    mats = []
    for b in range(len(ptr) - 1):
        lo, hi = ptr[b], ptr[b + 1]
        sel = (tgt >= lo) & (tgt < hi) & (tgt != src)
        mats.append(sp.coo_matrix((np.full(int(sel.sum()), 0.5), (tgt[sel] - lo, src[sel] - lo)), shape=(hi - lo, hi - lo)).tocsr())
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        if threadpool_limits is not None:
            with threadpool_limits(limits=16):
                for m in mats:
                    DBSCAN(eps=1.0, min_samples=MIN_SAMPLES, metric="precomputed", n_jobs=16).fit(m)
        else:
            for m in mats:
                DBSCAN(eps=1.0, min_samples=MIN_SAMPLES, metric="precomputed", n_jobs=16).fit(m)
        res["host_sklearn_dbscan_ms"] = round((time.perf_counter() - t0) * 1e3, 1)


def run_batch(events, nodes, a, dev):
    x, _y, batch, ptr = synth.make_events([nodes] * events, seed=1, device=dev)
    dm.register_batch(batch, ptr, events, max_nodes=nodes, min_nodes=nodes)
    pos = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1).contiguous()        # (eta, phi)
    N = pos.shape[0]
    density = nodes / (10.0 * 2 * math.pi)
    eps = math.sqrt((MEAN_HITS - 1) / (math.pi * density))

    def build():
        return dm.radius_table(pos, eps, batch, loop=True, max_num_neighbors=MAX_NBR + 1, int32_rows=True, period=PERIOD)

    table = build()
    nbr, cnt = table.nbr, table.cnt

    def cc():
        return _native._components(ptr, N, nbr=nbr, cnt=cnt)

    def db():
        return _native._components(ptr, N, nbr=nbr, cnt=cnt, min_samples=MIN_SAMPLES)

    def whole():
        return dm.dbscan(pos, eps, MIN_SAMPLES, batch, max_num_neighbors=MAX_NBR, period=PERIOD, return_core=True)

    labels, core = whole()
    dm.raise_deferred_errors()
    cc_labels, _c, _n, cc_flags = cc()
    entries = int(cnt.sum())
    res = {"events": events, "nodes": nodes, "eps": round(eps, 4), "min_samples": MIN_SAMPLES, "max_num_neighbors": MAX_NBR,
           "entries": entries, "mean_row": round(entries / N, 2), "max_row": int(cnt.max()),
           "clusters": int(labels.max()) + 1, "core_share": round(float(core.float().mean()), 3),
           "border_share": round(float((~core & (labels >= 0)).float().mean()), 3),
           "noise_share": round(float((labels < 0).float().mean()), 3),
           "components": int((cc_labels == torch.arange(N, device=dev)).sum()), "cc_flags": cc_flags.cpu().tolist(),
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for name, fn in (("radius_table", build), ("components_cc", cc), ("components_dbscan", db), ("dbscan_call", whole)):
        res[name + "_us"], res[name + "_spread_us"] = measure(fn, a.steps, a.warmup, a.repeats, dev)
    dm.raise_deferred_errors()
    read = 4 * entries + 4 * N
    res["cc_floor_us"] = round((read + 8 * N) / HBM_BYTES_PER_US, 2)
    res["dbscan_floor_us"] = round((read + 9 * N + 8 * events) / HBM_BYTES_PER_US, 2)
    res["cc_floor_share"] = round(res["cc_floor_us"] / res["components_cc_us"], 4)
    res["dbscan_floor_share"] = round(res["dbscan_floor_us"] / res["components_dbscan_us"], 4)
    if not a.no_host:
        host_reference(nbr, cnt, ptr, res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dbscan_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    for events, nodes in ((64, 4500), (128, 1000)):
        lines.append(run_batch(events, nodes, a, dev))
        print(json.dumps(lines[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

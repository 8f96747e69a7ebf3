"""Time of `condensation_cluster` and of its parts: the score op, the ranking launch (dmet_topk_f32 over all N slots), the
walk (csrc/condense.hip) and the whole call, against the same rule composed from torch operators.

    python tools/condense_step.py [--steps 50] [--warmup 10] [--repeats 5] [--json OUT] [--no-loop]

Input that looks like a trained object-condensation model, seeded: per event 20 .. 40 Gaussian blobs (sigma 0.15) in a
D = 3 cluster space of side 16, beta = 0.1 + 0.85 exp(-r^2 / 2 sigma^2) times a uniform factor in [0.7, 1] for a hit at
distance r from its blob's centre, and 10 % noise hits uniform in the box with beta below 0.08.  t_beta = 0.1, t_d = 0.8.
Coordinates are rounded to multiples of 1/64: every squared distance is then exact in fp32 however it is summed, so the
torch composition (which does not form the fmaf chain) must give EQUAL labels, and its time counts only if it does.
Batches: 64 x 4500, 128 x 1000, and a ragged one of 500 .. 8000 nodes an event with the first batch's total.  Two
extremes at 64 x 4500: `all_points` (a lattice of spacing 2 t_d, every beta above t_beta: every node its own condensation
point, the longest walk) and `coincident` (every node on one spot: one point an event).

Every part is timed by HIP events around the call, `steps` calls after `warmup`, the median of them; that is repeated
`repeats` times: `*_us` is the median of the medians, `*_spread_us` their largest minus their smallest.  The parts are
timed in loops of their own, not in turns.
`points_per_event` / `windows_per_event`: mean and largest; the windows are recounted on the host from the labels (a
window takes the next 64 candidates in rank order whose point was not found by an earlier window).
`floor_us`: one pass over beta, x and the outputs (4 + 4 D bytes read, 16 written per node, 8 per event) at the measured
copy bandwidth of the part (6.29 TB/s); `floor_share` = floor / measured kernel time.
`torch_loop_*`: the rule as a per-event loop of torch operators, one masked distance op and one host read per condensation
point, timed by the host clock around a synchronise over the first `torch_loop_events` events (all of them for the model-like
batches, one for `all_points`), one run after one warm-up run; `torch_loop_per_event_us` is that time over those events."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402
from deepmetv2_amd import _native  # noqa: E402

HBM_BYTES_PER_US = 6.29e6
T_BETA, T_D, D, SIGMA, SIDE, WINDOW = 0.1, 0.8, 3, 0.15, 16.0, 64


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


def model_like(sizes, seed):
    rng = np.random.default_rng(seed)
    betas, xs = [], []
    for n in sizes:
        blobs = int(rng.integers(20, 41))
        centre = rng.uniform(-SIDE / 2, SIDE / 2, (blobs, D))
        noise = rng.random(n) < 0.1
        which = rng.integers(0, blobs, n)
        x = centre[which] + rng.normal(0.0, SIGMA, (n, D))
        r2 = ((x - centre[which]) ** 2).sum(1)
        beta = (0.1 + 0.85 * np.exp(-r2 / (2 * SIGMA ** 2))) * rng.uniform(0.7, 1.0, n)
        x[noise] = rng.uniform(-SIDE / 2, SIDE / 2, (int(noise.sum()), D))
        beta[noise] = rng.uniform(0.0, 0.08, int(noise.sum()))
        betas.append(beta)
        xs.append(np.round(x * 64) / 64)
    return np.concatenate(betas).astype(np.float32), np.concatenate(xs).astype(np.float32)


def all_points(sizes, seed):
    rng = np.random.default_rng(seed)
    betas, xs = [], []
    for n in sizes:
        k = np.arange(n)
        xs.append(np.stack([k % 17, (k // 17) % 17, k // 289], 1) * (2 * T_D))
        betas.append(0.2 + 0.7 * rng.permutation(n) / n)                    # distinct: the torch loop's max has no tie
    return np.concatenate(betas).astype(np.float32), np.concatenate(xs).astype(np.float32)


def coincident(sizes, seed):
    rng = np.random.default_rng(seed)
    beta = np.concatenate([0.2 + 0.7 * rng.permutation(n) / n for n in sizes])
    return beta.astype(np.float32), np.full((sum(sizes), D), 0.25, dtype=np.float32)


def ragged_sizes(total, seed):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < total:
        sizes.append(int(rng.integers(500, 8001)))
    sizes[-1] -= sum(sizes) - total
    if sizes[-1] < 500:
        last = sizes.pop()
        sizes[-1] += last
    return sizes


def torch_loop(beta, x, ptr_host, events):
    """The rule from torch operators: per event, the best remaining candidate by one max (one host read), one masked
    distance op, two masked writes.  Labels numbered over the batch, for the first `events` events."""
    td2 = float(np.float32(T_D) * np.float32(T_D))
    hi_all = ptr_host[events]
    labels = torch.full((hi_all,), -1, dtype=torch.int64, device=beta.device)
    found = 0
    for b in range(events):
        lo, hi = ptr_host[b], ptr_host[b + 1]
        if hi == lo:
            continue
        xx, lab = x[lo:hi], labels[lo:hi]
        score = torch.where(beta[lo:hi] > T_BETA, beta[lo:hi], float("-inf"))
        iota = torch.arange(hi - lo, device=beta.device)
        while True:
            val = score.max()
            idx = torch.where(score == val, iota, hi - lo).min()            # ties to the lower index, as the rule has it
            v, i = torch.stack([val, idx.to(val.dtype)]).tolist()          # the host read of this point
            if v == float("-inf"):
                break
            i = int(i)
            take = (((xx - xx[i]) ** 2).sum(1) < td2) & (lab < 0)
            take[i] = True
            lab[take] = found
            score[take] = float("-inf")
            found += 1
    return labels


def windows_of(labels, beta, ptr_host):
    """(points, windows) per event, recounted on the host from batch-wide labels."""
    labels, beta = labels.cpu().numpy(), beta.cpu().numpy()
    points, windows = [], []
    for b in range(len(ptr_host) - 1):
        lo, hi = ptr_host[b], ptr_host[b + 1]
        lab, bt = labels[lo:hi], beta[lo:hi]
        cand = np.flatnonzero(bt > np.float32(T_BETA))
        cand = cand[np.lexsort((cand, -bt[cand].astype(np.float64)))]
        first = lab[lab >= 0].min() if (lab >= 0).any() else 0
        num = lab[cand] - first                         # the event-local number of every candidate's point, in rank order
        total = int(num.max()) + 1 if len(num) else 0
        found, cur, w = 0, 0, 0
        while cur < len(num):
            open_ = np.flatnonzero(num[cur:] >= found)[:WINDOW]
            if len(open_) == 0:
                break
            found = max(found, int(num[cur + open_].max()) + 1)
            cur += int(open_[-1]) + 1
            w += 1
        points.append(total)
        windows.append(w)
    return points, windows


def run_case(name, sizes, maker, loop_events, a, dev):
    beta_h, x_h = maker(sizes, seed=1)
    beta, x = torch.from_numpy(beta_h).to(dev), torch.from_numpy(x_h).to(dev)
    events, N = len(sizes), int(sum(sizes))
    ptr_host = [0] + np.cumsum(sizes).tolist()
    ptr = torch.tensor(ptr_host, dtype=torch.int64, device=dev)
    batch = torch.repeat_interleave(torch.arange(events, device=dev), torch.tensor(sizes, device=dev))
    dm.register_batch(batch, ptr, events, max_nodes=max(sizes), min_nodes=min(sizes))

    def score_op():
        return torch.where(beta > T_BETA, beta, float("-inf"))

    score = score_op()

    def ranking():
        return _native._topk(score, ptr, ptr, N)

    order, _map = ranking()

    def kernel():
        return _native._condense(beta, x, order, ptr, T_BETA, T_D)

    def whole():
        return dm.condensation_cluster(beta, x, batch, t_beta=T_BETA, t_d=T_D)

    labels = whole()
    dm.raise_deferred_errors()
    flags = kernel()[3].cpu().tolist()
    points, windows = windows_of(labels, beta, ptr_host)
    res = {"case": name, "events": events, "nodes": N, "min_event": min(sizes), "max_event": max(sizes), "D": D,
           "t_beta": T_BETA, "t_d": T_D, "flags": flags,
           "candidate_share": round(float((beta > T_BETA).float().mean()), 3),
           "noise_share": round(float((labels < 0).float().mean()), 3),
           "points_per_event": [round(statistics.mean(points), 1), max(points)],
           "windows_per_event": [round(statistics.mean(windows), 1), max(windows)],
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for part, fn in (("score_op", score_op), ("ranking", ranking), ("kernel", kernel), ("call", whole)):
        res[part + "_us"], res[part + "_spread_us"] = measure(fn, a.steps, a.warmup, a.repeats, dev)
    dm.raise_deferred_errors()
    res["floor_us"] = round(((4 + 4 * D + 16) * N + 8 * events) / HBM_BYTES_PER_US, 2)
    res["floor_share"] = round(res["floor_us"] / res["kernel_us"], 4)
    if not a.no_loop and loop_events:
        n = min(loop_events, events)
        torch_loop(beta, x, ptr_host, 1)                                    # warm-up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = torch_loop(beta, x, ptr_host, n)
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) * 1e6
        res["torch_loop_events"] = n
        res["torch_loop_equal"] = bool(torch.equal(got, labels[:ptr_host[n]]))
        if res["torch_loop_equal"]:                                         # its time counts only then
            res["torch_loop_us"] = round(dt, 1)
            res["torch_loop_per_event_us"] = round(dt / n, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("condense_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    total = 64 * 4500
    cases = (("model_64x4500", [4500] * 64, model_like, 64), ("model_128x1000", [1000] * 128, model_like, 128),
             ("model_ragged", ragged_sizes(total, 2), model_like, 10 ** 6), ("all_points", [4500] * 64, all_points, 1),
             ("coincident", [4500] * 64, coincident, 64))
    lines = []
    for name, sizes, maker, loop_events in cases:
        lines.append(run_case(name, sizes, maker, loop_events, a, dev))
        print(json.dumps(lines[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

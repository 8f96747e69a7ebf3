"""CPU model of the second kNN filter form's sweep (csrc/knn_filter.h, 32 features): how many candidates the exact
re-rank sees per query, how many rounds a wavefront's worst lane costs it, and how often a wavefront compacts its
entries -- with the main sweep's hit masks taken against tk[M-1] alone ("today") and against the running cut
min(tk[M-1], tk[k-1] + margin) (f2_running_tau).  numpy only, no GPU.

    python tools/knn_cut_model.py [--nodes 4500] [--k 16] [--case gaussian|clustered] [--seed 0] [--queries 2048]
                                  [--runcut both|on|off]

What is modelled: one event, keys |x_j|^2 - 2 x_i.x_j in float64, candidate tiles of 32 rows, wavefronts of 64
consecutive queries; the first 32 tiles deferred (kF2Defer: they only build the list of the M smallest tile minima and
are revisited against the final threshold); in the main sweep the threshold a tile's masks are taken against is the one
converted after the last odd tile at least two tiles back (the fold's operands are converted every second tile and the
next tile's products are issued before a tile's own update); one entry per tile with a non-zero mask, 30 slots per lane,
a wavefront compacts when any lane holds 29, a lane that keeps more than 27 overflows; the final threshold is
min(tau, f2_cut(tk[k-1])).  What is not: the fp16 operands, the fold's representable threshold (f2_tau16), the 11-bit
tile number inside an entry's minimum, split items, the second attempt.

sweep() returns per query the candidates that reach the re-rank; tests/test_knn_cut_model.py holds it to the property the
kernel's comment argues: the running cut never removes a candidate whose key is below the final threshold, and leaves
the final threshold as it was.
"""
import argparse

import numpy as np

SENTINEL = 1.0e10
TILE, WAVE, DEFER, SLOTS = 32, 64, 32, 30
CUT_SCALE = 1.25


def list_len(k):
    return k + 6 if k <= 16 else k + 4


def slack(an, rn, scale=1.0):
    return (2.0 * scale * (4e-5 * an * rn + 1e-5 * rn * rn + 4e-6 * an * an) + 1.96e-3 * an * rn + 6e-7 * (an + rn)
            + 6e-14 * rn * rn + 1e-12)


def cut(tkk, nx, scale=CUT_SCALE):
    """f2_cut at 32 features: the threshold that certifies d_k <= tkk + |x|^2 + slack, stretched by `scale`."""
    an = np.sqrt(nx) * 1.000001
    u0 = np.maximum(tkk + nx, 0.0)
    s = slack(an, an + np.sqrt(u0) * 1.00002)
    s = slack(an, an + np.sqrt(u0 + s) * 1.00002)
    U = u0 + s
    sl = slack(an, an + np.sqrt(U) * 1.00002)
    ts = U - nx + sl
    ts = ts + np.abs(ts) * (2.0 ** -15 + 4.8e-7) + (nx + sl) * 4.8e-7 + 2e-16
    return tkk + scale * (ts - tkk)


def make_event(case, nodes, seed, D=32):
    rng = np.random.default_rng(seed)
    if case == "gaussian":
        return rng.standard_normal((nodes, D))
    if case == "clustered":
        centres = 2.0 * rng.standard_normal((12, D))
        return centres[rng.integers(0, 12, nodes)] + 0.5 * rng.standard_normal((nodes, D))
    raise ValueError(case)


def _insert(tk, v):
    """the M smallest of (tk, v), sorted"""
    return np.sort(np.concatenate([tk, v[:, None]], axis=1), axis=1)[:, :tk.shape[1]]


def _wave(K, nx, k, runcut, scale):
    """One wavefront: K[64, T * 32] keys (+inf beyond the event).  Returns kept[64, T * 32], the final thresholds,
    the overflow flags, the number of compactions in the main sweep and the largest entry count seen."""
    Q, W = K.shape
    T, M = W // TILE, list_len(k)
    tmin = K.reshape(Q, T, TILE).min(axis=2)
    tk = np.full((Q, M), SENTINEL)
    bits = np.zeros((Q, SLOTS, TILE), dtype=bool)
    emin = np.full((Q, SLOTS), np.inf)
    etile = np.zeros((Q, SLOTS), dtype=np.int64)
    cnt = np.zeros(Q, dtype=np.int64)
    overflow = np.zeros(Q, dtype=bool)
    lanes = np.arange(Q)
    stat = {"compactions": 0, "peak": 0}

    def compact(tau, limit, count):
        nonlocal bits, emin, etile, cnt, overflow
        keep = (np.arange(SLOTS)[None, :] < cnt[:, None]) & ~(emin > tau[:, None])
        order = np.argsort(~keep, axis=1, kind="stable")          # kept entries first, in order
        bits = np.take_along_axis(bits, order[:, :, None], axis=1)
        emin = np.take_along_axis(emin, order, axis=1)
        etile = np.take_along_axis(etile, order, axis=1)
        cnt = keep.sum(axis=1)
        over = cnt > limit
        overflow |= over
        cnt[over] = 0
        stat["compactions"] += count

    def record(t, thr):
        nonlocal cnt
        m = K[:, t * TILE:(t + 1) * TILE] < np.where(overflow, -np.inf, thr)[:, None]
        slot = np.minimum(cnt, SLOTS - 1)
        bits[lanes, slot] = m
        emin[lanes, slot] = tmin[:, t]
        etile[lanes, slot] = t
        cnt = cnt + m.any(axis=1)
        stat["peak"] = max(stat["peak"], int(cnt.max()))

    t_def = min(T, DEFER)
    for t in range(t_def):
        tk = _insert(tk, tmin[:, t])
    tau = tk[:, M - 1].copy()
    margin = np.full(Q, np.inf)
    if runcut and scale is not None and t_def < T:
        tkk = tk[:, k - 1]
        with np.errstate(invalid="ignore", over="ignore"):
            m = cut(tkk, nx, scale) - tkk
        ok = (tkk < SENTINEL) & (m > 0.0) & np.isfinite(m)
        margin = np.where(ok, m * 1.01, np.inf)
        tau = np.minimum(tau, tkk + margin)
    conv = tau.copy()            # what the fold's operands hold
    thr = conv.copy()            # threshold of the tile this call records
    for s, t in enumerate(range(t_def, T)):
        if (cnt >= SLOTS - 1).any():
            compact(tau, SLOTS - 3, 1)
        nxt = conv.copy()        # the next tile's products are issued before this tile's update
        record(t, thr)
        tk = _insert(tk, tmin[:, t])
        last = tk[:, M - 1]
        if s % 2 == 1:           # CONV tile
            tau = np.minimum(last, tk[:, k - 1] + margin)
            conv = tau.copy()
        else:
            tau = last.copy()
        thr = nxt
    if scale is not None:
        tkk = tk[:, k - 1]
        with np.errstate(invalid="ignore", over="ignore"):
            c = cut(tkk, nx, scale)
        tau = np.where(tkk < SENTINEL, np.fmin(tau, c), tau)
    for t in range(t_def):       # the deferred tiles, against the final threshold
        if (cnt >= SLOTS - 1).any():
            compact(tau, SLOTS - 3, 0)
        record(t, tau)
    compact(tau, SLOTS, 0)
    kept = np.zeros((Q, W), dtype=bool)
    live = np.arange(SLOTS)[None, :] < cnt[:, None]
    for q in range(Q):
        for s_ in np.nonzero(live[q])[0]:
            t = etile[q, s_]
            kept[q, t * TILE:(t + 1) * TILE] |= bits[q, s_]
    return kept, tau, overflow, stat["compactions"], stat["peak"]


def sweep(x, queries, k=16, runcut=True, scale=CUT_SCALE):
    """Model the sweep of the first `queries` rows of the event x (a multiple of 64).  scale=None: no cut at all.
    Returns dict(kept[q, n] bool, tau[q], overflow[q], keys[q, n], compactions[w], peak[w])."""
    n = x.shape[0]
    assert queries % WAVE == 0 and queries <= n
    T = (n + TILE - 1) // TILE
    x = np.asarray(x, dtype=np.float64)
    nrm = (x * x).sum(axis=1)
    out = {"kept": [], "tau": [], "overflow": [], "keys": [], "compactions": [], "peak": []}
    for w in range(queries // WAVE):
        q = slice(w * WAVE, (w + 1) * WAVE)
        K = np.full((WAVE, T * TILE), np.inf)
        K[:, :n] = nrm[None, :] - 2.0 * (x[q] @ x.T)
        kept, tau, over, ncomp, peak = _wave(K, nrm[q], k, runcut, scale)
        out["kept"].append(kept[:, :n]); out["tau"].append(tau); out["overflow"].append(over)
        out["keys"].append(K[:, :n]); out["compactions"].append(ncomp); out["peak"].append(peak)
    return {name: (np.concatenate(v) if name in ("kept", "tau", "overflow", "keys") else np.array(v))
            for name, v in out.items()}


def row(label, r):
    cand = r["kept"].sum(axis=1)
    worst = cand.reshape(-1, WAVE).max(axis=1)
    return (f"| {label} | {cand.mean():.1f} | {worst.mean():.1f} | {r['compactions'].mean():.2f} | {int(r['peak'].max())} | "
            f"{int(r['overflow'].sum())} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=4500)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--case", choices=["gaussian", "clustered"], default="gaussian")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--runcut", choices=["both", "on", "off"], default="both")
    a = ap.parse_args()
    x = make_event(a.case, a.nodes, a.seed)
    print(f"{a.nodes} nodes, k = {a.k}, {a.case}, seed {a.seed}, {a.queries} queries")
    print("| | candidates re-ranked per query (mean) | mean over wavefronts of the worst lane (= re-rank rounds) | "
          "in-sweep compactions per wavefront | most entries in a lane | overflowed queries |")
    print("|---|---|---|---|---|---|")
    if a.runcut in ("both", "off"):
        print(row("today (tau = tk[M-1])", sweep(x, a.queries, a.k, runcut=False)))
    if a.runcut in ("both", "on"):
        print(row("running cut min(tk[M-1], tk[k-1] + margin)", sweep(x, a.queries, a.k, runcut=True)))


if __name__ == "__main__":
    main()

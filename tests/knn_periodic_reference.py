"""Exact numpy restatement of the periodic kNN table (include/dmet.h, dmet_knn_periodic_f32).

The squared distance of a pair is the fp32 chain of the periodic radius graph (radius_periodic_reference.pair_d2: a
periodic coordinate's difference is wrapped as a = |d|; a = (a > L/2) ? L - a : a before it enters fmaf(a, a, acc)).
Row i keeps the k candidates of its event with the smallest (d, j), ties to the lower j (R2); a candidate at d >= 1e10
or NaN is never selected; empty slots are (-1, 1e10).  With period None this is the K1 contract of dmet_knn_f32.
"""
from __future__ import annotations

import numpy as np

from radius_periodic_reference import F32, pair_d2

SENTINEL = F32(1e10)


def knn_table(x, ptr, k: int, period):
    """(nbr[N, k] int32 global ids, -1 padded; dist[N, k] fp32, 1e10 padded; loc[N, k] uint16 event-local ids, 0xFFFF
    padded)."""
    x = np.asarray(x, dtype=F32)
    ptr = np.asarray(ptr, dtype=np.int64)
    N = x.shape[0]
    nbr = np.full((N, k), -1, dtype=np.int32)
    dist = np.full((N, k), SENTINEL, dtype=F32)
    loc = np.full((N, k), 0xFFFF, dtype=np.uint16)
    for b in range(len(ptr) - 1):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        n = hi - lo
        if n == 0:
            continue
        xe = x[lo:hi]
        j = np.arange(n)
        for i0 in range(0, n, 512):                       # row blocks keep the pair matrix small
            i1 = min(i0 + 512, n)
            d2 = pair_d2(xe[i0:i1, None, :], xe[None, :, :], period)
            for ii in range(i0, i1):
                d = d2[ii - i0]
                ok = np.flatnonzero(d < SENTINEL)          # NaN compares false: never selected
                order = ok[np.lexsort((j[ok], d[ok]))][:k]
                m = len(order)
                nbr[lo + ii, :m] = order + lo
                dist[lo + ii, :m] = d[order]
                loc[lo + ii, :m] = order
    return nbr, dist, loc


def circular_d2_f64(x, period):
    """float64 squared distances of all pairs of one event with the true circular difference (geometry checks)."""
    x = np.asarray(x, dtype=np.float64)
    acc = np.zeros((x.shape[0], x.shape[0]))
    for c in range(x.shape[1]):
        d = np.abs(x[None, :, c] - x[:, None, c])
        L = 0.0 if period is None or period[c] is None else float(F32(period[c]))
        if L > 0:
            d = np.mod(d, L)
            d = np.minimum(d, L - d)
        acc += d * d
    return acc

"""Exact numpy restatement of farthest point sampling (include/dmet.h, dmet_fps_f32).

Event b owns the nodes ptr[b] .. ptr[b+1]-1 and yields m[b] global ids.  The squared distance of point p and pick s is
radius_periodic_reference.pair_d2(xe, xe[s], None): a = x[s,c] - x[p,c], acc = fmaf(a, a, acc) in coordinate order, fp32.
    out[0]  = lo + clamp(start[b], 0, n-1);  dist = d(., start)
    out[i]  = lo + np.argmax(dist)           (the FIRST maximum: ties go to the lowest index)
    dist    = np.minimum(dist, d(., s))
m[b] > n is legal: once every distinct point is taken every distance is 0 and index 0 repeats.
"""
from __future__ import annotations

import numpy as np

from radius_periodic_reference import F32, pair_d2


def sample_counts(ptr, ratio) -> np.ndarray:
    """m[B] = ceil(fp32(n_b) * fp32(ratio_b)), the product rounded to fp32 (ratio: a float or a [B] / 1-element array)."""
    n = np.diff(np.asarray(ptr, dtype=np.int64)).astype(F32)
    r = np.asarray(ratio, dtype=F32).reshape(-1)
    return np.maximum(np.ceil((n * r).astype(F32)).astype(np.int64), 0)


def fps(x, ptr, m, start=None) -> np.ndarray:
    """int64 [sum(m)]: the picks of every event as global node ids, events in order."""
    x = np.asarray(x, dtype=F32)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    ptr = np.asarray(ptr, dtype=np.int64)
    B = len(ptr) - 1
    m = np.asarray(m, dtype=np.int64).reshape(-1)
    start = np.zeros(B, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64).reshape(-1)
    assert len(m) == B and len(start) == B
    out = []
    for b in range(B):
        lo, n = int(ptr[b]), int(ptr[b + 1] - ptr[b])
        if n == 0 or m[b] <= 0:
            continue
        xe = x[lo:lo + n]
        s = int(min(max(start[b], 0), n - 1))
        picks = np.empty(int(m[b]), dtype=np.int64)
        picks[0] = s
        dist = pair_d2(xe, xe[s], None)
        for i in range(1, int(m[b])):
            s = int(np.argmax(dist))
            picks[i] = s
            dist = np.minimum(dist, pair_d2(xe, xe[s], None))
        out.append(picks + lo)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)

"""Exact numpy restatement of the periodic radius graph (include/dmet.h, dmet_radius_periodic_f32).

For every pair (i, j) of an event the squared distance is the fp32 chain in coordinate order:
    d   = x[j,c] - x[i,c]                        (fp32)
    a   = |d|;  a = (a > 0.5f * L) ? L - a : a   (fp32, periodic coordinates only; plain ones keep a = d)
    acc = fmaf(a, a, acc)
A hit is acc < fp32(r) * fp32(r) (fp32 product); row i keeps the first max_nbr hits in ascending j, and skip_self counts
node i towards the cap without storing it.

numpy has no fused multiply-add: a*a is exact in float64 (24 + 24 bits), the sum with acc is made exact by TwoSum, and
round-to-odd to 53 bits followed by the cast to fp32 (round to nearest even) is the correctly rounded fp32 fma.
`fraction_pair_d2` restates one pair with fractions.Fraction, to pin this arithmetic.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

F32 = np.float32


def _fma32(a: np.ndarray, acc: np.ndarray) -> np.ndarray:
    """fp32 fmaf(a, a, acc), elementwise, exact."""
    p = a.astype(np.float64) * a.astype(np.float64)        # exact
    q = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + q
        bb = s - p
        err = (p - (s - bb)) + (q - bb)                       # p + q = s + err exactly (finite s)
        bits = s.view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)   # round to odd
        return s.astype(F32)


def wrap(d: np.ndarray, L: float) -> np.ndarray:
    """The periodic difference of the contract, fp32."""
    L = F32(L)
    a = np.abs(d.astype(F32))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(a > F32(0.5) * L, (L - a).astype(F32), a).astype(F32)


def pair_d2(xi: np.ndarray, xj: np.ndarray, period) -> np.ndarray:
    """Squared distances of broadcast pairs: xi[..., D], xj[..., D] fp32 -> fp32 [...]."""
    xi = np.asarray(xi, dtype=F32)
    xj = np.asarray(xj, dtype=F32)
    shape = np.broadcast_shapes(xi.shape, xj.shape)[:-1]
    acc = np.zeros(shape, dtype=F32)
    D = xi.shape[-1]
    for c in range(D):
        with np.errstate(invalid="ignore", over="ignore"):
            d = (xj[..., c] - xi[..., c]).astype(F32)
        L = 0.0 if period is None or period[c] is None else float(F32(period[c]))
        a = wrap(d, L) if L > 0 else d
        acc = _fma32(a, acc)
    return acc


def radius_hits(x, ptr, r: float, period) -> list:
    """Every hit of every node, uncapped: a list of N int64 arrays of global ids in ascending order."""
    x = np.asarray(x, dtype=F32)
    ptr = np.asarray(ptr, dtype=np.int64)
    r32 = F32(r)
    r2 = F32(r32 * r32)
    hits = [np.zeros(0, dtype=np.int64)] * x.shape[0]
    for b in range(len(ptr) - 1):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        xe = x[lo:hi]
        for i0 in range(0, hi - lo, 512):                 # row blocks keep the pair matrix small
            i1 = min(i0 + 512, hi - lo)
            hit = pair_d2(xe[i0:i1, None, :], xe[None, :, :], period) < r2
            for ii in range(i0, i1):
                hits[lo + ii] = np.flatnonzero(hit[ii - i0]) + lo
    return hits


def cap(hits: list, max_nbr: int, skip_self: bool = False):
    """(nbr[N, max_nbr] int32, -1 beyond cnt; cnt[N] int32): the first max_nbr hits of each row, node i counted towards
    the cap but not stored when skip_self."""
    N = len(hits)
    nbr = np.full((N, max_nbr), -1, dtype=np.int32)
    cnt = np.zeros(N, dtype=np.int32)
    for i, h in enumerate(hits):
        js = h[:max_nbr]
        if skip_self:
            js = js[js != i]
        cnt[i] = len(js)
        nbr[i, :len(js)] = js
    return nbr, cnt


def radius_table(x, ptr, r: float, max_nbr: int, period, skip_self: bool = False):
    """(nbr[N, max_nbr] int32 global ids, -1 beyond cnt; cnt[N] int32) of the periodic radius graph."""
    return cap(radius_hits(x, ptr, r, period), max_nbr, skip_self)


# ---- the same arithmetic with exact rationals (pins the float64 / TwoSum restatement) ----------------------------
def round_f32(v: Fraction) -> float:
    """Round an exact rational to the nearest fp32 (ties to even), overflow to inf."""
    if v == 0:
        return 0.0
    sign = -1 if v < 0 else 1
    m = abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    while Fraction(2) ** (e + 1) <= m:
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q, rem = divmod(m, ulp)
    if rem * 2 > ulp or (rem * 2 == ulp and q % 2 == 1):
        q += 1
    out = q * ulp
    if out >= Fraction(2) ** 128:
        return sign * float("inf")
    return sign * float(out)


def fraction_pair_d2(xi, xj, period) -> float:
    """One pair's squared distance with every fp32 operation done exactly and rounded once (finite inputs)."""
    acc = Fraction(0)
    for c in range(len(xi)):
        d = Fraction(round_f32(Fraction(float(F32(xj[c]))) - Fraction(float(F32(xi[c])))))
        L = 0.0 if period is None or period[c] is None else float(F32(period[c]))
        if L > 0:
            a = abs(d)
            if a > Fraction(L) / 2:
                a = Fraction(round_f32(Fraction(L) - a))
            d = a
        acc = Fraction(round_f32(d * d + acc))
    return float(acc)

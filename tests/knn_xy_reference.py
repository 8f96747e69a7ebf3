"""Exact numpy restatement of the two-set tables (include/dmet.h, dmet_knn_xy_f32 / dmet_radius_xy_f32), and a CPU
stand-in for the `_native` entries of the two-set operators (test infrastructure, installed explicitly by the host tests).

Queries are the rows of y, candidates the rows of x of the same event.  The squared distance of query i and candidate j
is radius_periodic_reference.pair_d2(y[i], x[j], period): d = x[j,c] - y[i,c], wrapped on a periodic coordinate, squared
into the fp32 fma chain in coordinate order.
  kNN:    row i keeps the k candidates with the smallest (d, j), ties to the lower j; d >= 1e10 or NaN is never selected;
          empty slots are (-1, 1e10).
  radius: row i keeps the first max_nbr candidates in ascending j with d < fp32(r) * fp32(r); cnt[i] of them.
There is no self to exclude: the two sets have separate index spaces.
"""
from __future__ import annotations

import numpy as np
import torch

from radius_periodic_reference import F32, pair_d2

SENTINEL = F32(1e10)
ROWS = 512          # query rows per block: keeps the pair matrix small


def _blocks(x, ptr_x, y, ptr_y, period):
    """(first query, last query + 1, first candidate, d2 [rows, nx]) for every block of queries of every event that has
    both queries and candidates."""
    x = np.asarray(x, dtype=F32)
    y = np.asarray(y, dtype=F32)
    ptr_x = np.asarray(ptr_x, dtype=np.int64)
    ptr_y = np.asarray(ptr_y, dtype=np.int64)
    assert len(ptr_x) == len(ptr_y)
    for b in range(len(ptr_y) - 1):
        xl, xh, yl, yh = int(ptr_x[b]), int(ptr_x[b + 1]), int(ptr_y[b]), int(ptr_y[b + 1])
        if xh == xl or yh == yl:
            continue
        xe = x[xl:xh]
        for i0 in range(yl, yh, ROWS):
            i1 = min(i0 + ROWS, yh)
            yield i0, i1, xl, pair_d2(y[i0:i1, None, :], xe[None, :, :], period)


def knn_table(x, ptr_x, y, ptr_y, k: int, period=None):
    """(nbr[Ny, k] int32 ids into x, -1 padded; dist[Ny, k] fp32, 1e10 padded)."""
    Ny = np.asarray(y).shape[0]
    nbr = np.full((Ny, k), -1, dtype=np.int32)
    dist = np.full((Ny, k), SENTINEL, dtype=F32)
    for i0, i1, xl, d2 in _blocks(x, ptr_x, y, ptr_y, period):
        j = np.arange(d2.shape[1])
        for ii in range(i0, i1):
            d = d2[ii - i0]
            ok = np.flatnonzero(d < SENTINEL)              # NaN compares false: never selected
            order = ok[np.lexsort((j[ok], d[ok]))][:k]
            nbr[ii, :len(order)] = order + xl
            dist[ii, :len(order)] = d[order]
    return nbr, dist


def radius_table(x, ptr_x, y, ptr_y, r: float, max_nbr: int, period=None):
    """(nbr[Ny, max_nbr] int32 ids into x, -1 beyond cnt; cnt[Ny] int32)."""
    Ny = np.asarray(y).shape[0]
    r32 = F32(r)
    r2 = F32(r32 * r32)
    nbr = np.full((Ny, max_nbr), -1, dtype=np.int32)
    cnt = np.zeros(Ny, dtype=np.int32)
    for i0, i1, xl, d2 in _blocks(x, ptr_x, y, ptr_y, period):
        hit = d2 < r2
        for ii in range(i0, i1):
            js = np.flatnonzero(hit[ii - i0])[:max_nbr]
            cnt[ii] = len(js)
            nbr[ii, :len(js)] = js + xl
    return nbr, cnt


def edges_of(nbr):
    """int64 [2, E] of a table's valid slots: row 0 = query, row 1 = candidate, in table order."""
    nbr = np.asarray(nbr)
    q, s = np.nonzero(nbr >= 0)
    return np.stack([q.astype(np.int64), nbr[q, s].astype(np.int64)])


# ---- CPU stand-in for deepmetv2_amd._native's two-set entries ------------------------------------------------------
def _period(period):
    return None if period is None else [None if p == 0 else p for p in period]


def knn_xy(x, ptr_x, y, ptr_y, k, period=None):
    nbr, dist = knn_table(x.detach().numpy(), ptr_x.numpy(), y.detach().numpy(), ptr_y.numpy(), k, _period(period))
    return torch.from_numpy(nbr), torch.from_numpy(dist)


def radius_xy(x, ptr_x, y, ptr_y, r, max_nbr, period=None, pad=True):
    nbr, cnt = radius_table(x.detach().numpy(), ptr_x.numpy(), y.detach().numpy(), ptr_y.numpy(), r, max_nbr,
                            _period(period))
    nbr, cnt = torch.from_numpy(nbr), torch.from_numpy(cnt)
    if not pad:     # the counted form leaves slots >= cnt unwritten: poison them so that a consumer reading them fails
        slot = torch.arange(max_nbr, dtype=torch.int32).view(1, -1)
        nbr = torch.where(slot < cnt.view(-1, 1), nbr, torch.full_like(nbr, 2 ** 30))
    return nbr, cnt


def edge_features_xy(x_src, x_dst, src, tgt):
    assert src.numel() == 0 or (0 <= int(src.min()) and int(src.max()) < x_src.shape[0])
    assert tgt.numel() == 0 or (0 <= int(tgt.min()) and int(tgt.max()) < x_dst.shape[0])
    xi = x_dst[tgt.long()]
    return torch.cat([xi, x_src[src.long()] - xi], 1)


def edge_features_xy_bwd(g_feat, rowptr, srcptr, srcperm, N_src, N_dst, H, want_src=True, want_dst=True):
    E = int(rowptr[-1])
    g_dst = g_src = None
    if want_dst:
        tgt = torch.repeat_interleave(torch.arange(N_dst), (rowptr[1:] - rowptr[:-1]).long())
        g_dst = torch.zeros((N_dst, H), dtype=g_feat.dtype).index_add_(0, tgt, g_feat[:E, :H] - g_feat[:E, H:])
    if want_src:
        src = torch.repeat_interleave(torch.arange(N_src), (srcptr[1:] - srcptr[:-1]).long())
        g_src = torch.zeros((N_src, H), dtype=g_feat.dtype).index_add_(0, src, g_feat[srcperm[:E].long(), H:])
    return g_src, g_dst


def install(monkeypatch):
    """fake_native's stand-ins plus the four two-set entries above."""
    import fake_native
    import deepmetv2_amd._native as nat
    fake_native.install(monkeypatch)
    g = globals()
    for n in ("knn_xy", "radius_xy", "edge_features_xy", "edge_features_xy_bwd"):
        monkeypatch.setattr(nat, n, g[n])

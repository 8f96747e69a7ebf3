"""TEST INFRASTRUCTURE: an oracle-backed stand-in for deepmetv2_amd._native so that the HOST logic (autograd
wiring, graph registries, argument checks, DDP sharding) can be exercised in a GPU-less container.

Never shipped or imported by the package: tests install it explicitly with `install(monkeypatch)`.  Every function
restates the contract of the C-ABI entry point of the same name (include/dmet.h) with plain torch on the CPU.
"""
from __future__ import annotations

import torch

from oracle import ref_ops


def knn(x, ptr, k):
    return ref_ops.knn_table(x, ptr, k)


def knn_local(x, ptr, k, stats=None):
    nbr, dist = ref_ops.knn_table(x, ptr, k)
    counts = (ptr[1:] - ptr[:-1]).long()
    lo = torch.repeat_interleave(ptr[:-1], counts).to(torch.int32).view(-1, 1)
    loc = torch.where(nbr >= 0, nbr - lo, torch.full_like(nbr, 0xFFFF))
    loc = torch.where(loc >= 0x8000, loc - 0x10000, loc).to(torch.int16)      # uint16 payload in an int16 tensor
    return nbr, dist, loc


def radius(x, ptr, r, max_nbr, skip_self=False, pad=True, local=False, int32_rows=True):
    import ctypes  # noqa: F401
    if local:
        nbr, cnt = radius(x, ptr, r, max_nbr, skip_self, pad)
        stride16 = (max_nbr + 7) // 8 * 8
        counts = (ptr[1:] - ptr[:-1]).long()
        lo = torch.repeat_interleave(ptr[:-1], counts).view(-1, 1)
        slot = torch.arange(stride16).view(1, -1)
        loc = torch.zeros((nbr.shape[0], stride16), dtype=torch.long)
        loc[:, :max_nbr] = nbr.long() - lo
        c = cnt.long().view(-1, 1)
        loc = torch.where(slot < c, loc, torch.full_like(loc, 0xFFFF))       # pad of the last chunk
        loc = torch.where(slot < (c + 7) // 8 * 8, loc, torch.full_like(loc, 0x1234))   # unwritten: poison
        loc &= 0xFFFF
        return (nbr if (int32_rows or pad) else None), cnt, torch.where(loc >= 0x8000, loc - 0x10000, loc).to(torch.int16)
    x = x.detach().float().contiguous()
    N, D = x.shape
    nbr = torch.empty((N, max_nbr), dtype=torch.int32)
    cnt = torch.empty((N,), dtype=torch.int32)
    rc = ref_ops.lib().dmet_oracle_radius_f32(x.data_ptr(), ptr.contiguous().data_ptr(), ptr.numel() - 1, D, float(r),
                                              max_nbr, nbr.data_ptr(), cnt.data_ptr())
    assert rc == 0
    if skip_self:   # upstream's loop=False: the node counts towards the limit but is not stored
        self_id = torch.arange(N, dtype=torch.int32).view(-1, 1)
        keep = (nbr != self_id) & (nbr >= 0)
        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)
        nbr = torch.gather(torch.where(keep, nbr, torch.full_like(nbr, -1)), 1, order)
        cnt = keep.sum(1).to(torch.int32)
    if not pad:   # the counted form leaves slots >= cnt unwritten: poison them so that a consumer reading them fails
        slot = torch.arange(max_nbr, dtype=torch.int32).view(1, -1)
        nbr = torch.where(slot < cnt.view(-1, 1), nbr, torch.full_like(nbr, 2 ** 30))
    return nbr, cnt


def node_linear_split(x, W, b, sliced=False):   # the stand-in keeps row-major tables either way
    H = x.shape[1]
    Wd = W[:, :H] - W[:, H:]
    P = x @ Wd.t()
    if b is not None:
        P = P + b
    return P.detach(), (x @ W[:, H:].t()).detach()


def gather_max(P, Q, nbr, ptr, want_arg, cnt=None, lds=False, nbr_local=None, sliced=False, mixed=False, max_nodes=None):
    if nbr_local is not None:
        # the local table must describe the same graph (this is what the uint16 kernel would gather)
        counts = (ptr[1:] - ptr[:-1]).long()
        lo = torch.repeat_interleave(ptr[:-1], counts).to(torch.int32).view(-1, 1)
        u = nbr_local.to(torch.int32) & 0xFFFF
        assert torch.equal(torch.where(u == 0xFFFF, torch.full_like(u, -1), u + lo), nbr)
    N, H = P.shape
    k = nbr.shape[1]
    if cnt is not None:   # counted tables: slots >= cnt[i] are undefined
        slot = torch.arange(k, dtype=torch.int32).view(1, -1)
        nbr = torch.where(slot < cnt.view(-1, 1), nbr, torch.full_like(nbr, -1))
    idx = nbr.long().clamp(min=0)
    vals = Q[idx]                                             # [N,k,H]
    vals = torch.where((nbr >= 0).unsqueeze(-1), vals, torch.full_like(vals, float("-inf")))
    best, arg = vals.max(dim=1)
    # lowest slot on ties: torch.max returns the first maximal index on CPU
    first = (vals == best.unsqueeze(1)).float().argmax(dim=1)
    any_valid = (nbr >= 0).any(dim=1, keepdim=True)
    out = torch.where(any_valid, P + best, torch.zeros_like(P))
    arg8 = torch.where(any_valid, first, torch.full_like(first, 255)).to(torch.uint8)
    return out, (arg8 if want_arg else None)


def edgeconv_fused_lds(x, W, b, nbr, ptr, want_arg):
    P, Q = node_linear_split(x, W, b)
    return gather_max(P, Q, nbr, ptr, want_arg)


def reverse_index(keys, num_keys):
    keys = keys.reshape(-1)
    M = keys.numel()
    k64 = keys.long()
    k64 = torch.where((k64 < 0) | (k64 >= num_keys), torch.full_like(k64, num_keys), k64)
    order = torch.sort(k64, stable=True).indices
    counts = torch.bincount(k64, minlength=num_keys + 1)[:num_keys]
    rev_ptr = torch.zeros(num_keys + 1, dtype=torch.int32)
    rev_ptr[1:] = counts.cumsum(0).int()
    return rev_ptr, order.int() if M else torch.zeros(1, dtype=torch.int32)


def gather_max_bwd(g_out, arg, rev_ptr, rev_slot, k):
    N, H = g_out.shape
    gQ = torch.zeros_like(g_out)
    n_valid = int(rev_ptr[-1])
    # recover (source j, position e) pairs from the reverse index
    src = torch.repeat_interleave(torch.arange(N), (rev_ptr[1:] - rev_ptr[:-1]).long())
    e = rev_slot[:n_valid].long()
    i, s = e // k, e % k
    contrib = torch.where(arg[i].long() == s.view(-1, 1), g_out[i], torch.zeros_like(g_out[i]))
    gQ.index_add_(0, src, contrib)
    return gQ


def edge_features(x, src, tgt):
    xi, xj = x[tgt.long()], x[src.long()]
    return torch.cat([xi, xj - xi], dim=1).detach()


def edge_features_bwd(g_feat, rowptr, srcptr, srcperm, N, H):
    E = g_feat.shape[0]
    tgt = torch.repeat_interleave(torch.arange(N), (rowptr[1:] - rowptr[:-1]).long())
    src_of = torch.empty(E, dtype=torch.long)
    src_nodes = torch.repeat_interleave(torch.arange(N), (srcptr[1:] - srcptr[:-1]).long())
    src_of[srcperm[:E].long()] = src_nodes
    gx = torch.zeros((N, H), dtype=g_feat.dtype)
    gx.index_add_(0, tgt, g_feat[:, :H] - g_feat[:, H:])
    gx.index_add_(0, src_of, g_feat[:, H:])
    return gx


def _tgt_of(rowptr, N):
    return torch.repeat_interleave(torch.arange(N), (rowptr[1:] - rowptr[:-1]).long())


def segment_max(msg, rowptr, N):
    out, arg = ref_ops.scatter_max(msg.detach(), _tgt_of(rowptr, N), N)
    E = msg.shape[0]
    return out, torch.where(arg >= E, torch.full_like(arg, -1), arg).int()


def segment_sum(msg, rowptr, N):
    return ref_ops.scatter_add(msg.detach(), _tgt_of(rowptr, N), dim_size=N)


def segment_max_bwd(g_out, arg, rowptr, E):
    N, H = g_out.shape
    tgt = _tgt_of(rowptr, N)
    won = arg.long()[tgt] == torch.arange(E).view(-1, 1)
    return torch.where(won, g_out[tgt], torch.zeros((E, H), dtype=g_out.dtype))


def segment_sum_bwd(g_out, rowptr, E):
    return g_out[_tgt_of(rowptr, g_out.shape[0])].clone()


def met_reduce(w, x, ptr):
    B = ptr.numel() - 1
    batch = torch.repeat_interleave(torch.arange(B), ptr.diff())
    met = torch.zeros((B, 2), dtype=torch.float32)
    met.index_add_(0, batch, w.detach().view(-1, 1) * x[:, :2])
    return met


def met_reduce_bwd(g_met, x, ptr, scale=None):
    B = ptr.numel() - 1
    batch = torch.repeat_interleave(torch.arange(B), ptr.diff())
    if scale is not None:
        g_met = g_met * scale
    return g_met[batch, 0] * x[:, 0] + g_met[batch, 1] * x[:, 1]


def segment_sum_1d(src, ptr):
    B = ptr.numel() - 1
    batch = torch.repeat_interleave(torch.arange(B), ptr.diff())
    return torch.zeros(B, dtype=src.dtype).index_add_(0, batch, src.detach())


def batch_to_ptr(batch, B):
    """The kernel's own rule, not the oracle's: no check of the vector.  Position i (0..N) writes ptr[b] = i for every
    b in [max(batch[i-1] + 1, 0), min(batch[i], B)] (batch[-1] = -1, batch[N] = B); every entry gets written.  On an
    unsorted vector several positions write one entry and the device gives no order: the last writer wins here."""
    v = torch.cat([torch.tensor([-1]), batch.long().cpu(), torch.tensor([B])])
    ptr = torch.full((B + 1,), -1, dtype=torch.int64)
    for i in torch.nonzero(v[1:] > v[:-1]).view(-1).tolist():
        lo, hi = max(int(v[i]) + 1, 0), min(int(v[i + 1]), B)
        if lo <= hi:
            ptr[lo:hi + 1] = i
    assert bool((ptr >= 0).all())
    return ptr


def xty(A, Bm):
    return (A.detach().t() @ Bm.detach()).contiguous()


def onehot_xty(index, Bm, num_rows):
    return torch.zeros((num_rows, Bm.shape[1]), dtype=Bm.dtype).index_add_(0, index, Bm.detach())


def _encode_chain(x_cont, x_cat, params):
    if x_cat.is_floating_point():   # lazy categorical columns: the kernel truncates like .long()
        x_cat = x_cat.long()
    Wc, bc, Wk, bk, Wa, ba, Echg, Epdg, Epv = params
    F = torch.nn.functional
    pdg = x_cat[:, 0].abs()
    for cls, val in enumerate((1, 2, 11, 13, 22, 130, 211)):
        pdg = torch.where(pdg == val, torch.full_like(pdg, cls), pdg)
    cat = torch.cat([Echg[x_cat[:, 1] + 1], Epdg[pdg], Epv[x_cat[:, 2]]], dim=1)
    e_cat = F.elu(F.linear(cat, Wk, bk))
    e_cont = F.elu(F.linear(x_cont, Wc, bc))
    return F.elu(F.linear(torch.cat([e_cat, e_cont], dim=1), Wa, ba))


def encode_fwd(x_cont, x_cat, params):
    with torch.no_grad():
        return _encode_chain(x_cont, x_cat, params)


def encode_bwd(x_cont, x_cat, params, h, g_h):
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    with torch.enable_grad():
        out = _encode_chain(x_cont, x_cat, ps)
    return list(torch.autograd.grad(out, ps, g_h))


def bn_fwd(x, residual, gamma, beta, eps, momentum, running_mean, running_var, training, num_batches_tracked=None):
    if training and num_batches_tracked is not None:
        num_batches_tracked.add_(1)
    if training:
        mean = x.mean(0)
        var = x.var(0, unbiased=False)
        if running_mean is not None:
            n = x.shape[0]
            running_mean.mul_(1 - momentum).add_(momentum * mean)
            running_var.mul_(1 - momentum).add_(momentum * var * n / max(n - 1, 1))
    else:
        mean, var = running_mean.clone(), running_var.clone()
    invstd = (var + eps).rsqrt()
    y = (x - mean) * (gamma * invstd) + beta
    if residual is not None:
        y = y + residual
    return y, mean, invstd


def bn_bwd(x, g_y, gamma, mean, invstd):
    xh = (x - mean) * invstd
    g_b = g_y.sum(0)
    g_w = (g_y * xh).sum(0)
    n = x.shape[0]
    g_x = gamma * invstd * (g_y - g_b / n - xh * (g_w / n))
    return g_x, g_w, g_b


def _to_sliced(gQ):     # [N,32] -> the slice-major [8,N,4] layout of dmet_gather_max_bwd_sliced_f32
    return gQ.view(gQ.shape[0], 8, 4).permute(1, 0, 2).contiguous()


def edgeconv_linear_bwd(x, weight, g_out, arg, gQ, want_bias=True, g_add=None, gq_sliced=False):
    H = x.shape[1]
    if gq_sliced:
        gQ = gQ.permute(1, 0, 2).reshape(x.shape[0], 32)
    none = 255 if (arg is not None and arg.dtype == torch.uint8) else 0xFFFF
    gP = g_out if arg is None else g_out * ((arg.long() & 0xFFFF) != none).to(g_out.dtype)
    Wd, W2 = weight[:, :H] - weight[:, H:], weight[:, H:]
    gx = gP @ Wd + gQ @ W2
    if g_add is not None:
        gx = gx + g_add
    gWd = gP.t() @ x
    gW = torch.cat([gWd, gQ.t() @ x - gWd], dim=1)
    return gx, gW, (gP.sum(0) if want_bias else None)


def gather_max_bwd_lds(g_out, arg, nbr, ptr, nbr_local=None, max_nodes=None, sliced=False):
    N, H = g_out.shape
    gQ = torch.zeros_like(g_out)
    a = arg.long()
    valid = a != 255
    j = torch.gather(nbr.long(), 1, a.clamp(max=nbr.shape[1] - 1))        # [N,H] winner source per channel
    cols = torch.arange(H).expand(N, H)
    gQ.index_put_((j[valid], cols[valid]), g_out[valid], accumulate=True)
    return _to_sliced(gQ) if (sliced and H == 32) else gQ


def met_loss(met, truth):
    r = met + truth[:, :2]
    return 0.5 * (r * r).sum(1).mean().view(1), r / met.shape[0]


def _head_chain(emb, params):
    W1, b1, W2, b2 = params
    F = torch.nn.functional
    return torch.sigmoid(F.linear(F.elu(F.linear(emb, W1, b1)), W2, b2)).squeeze(-1)


def head_fwd(emb, params):
    with torch.no_grad():
        return _head_chain(emb, params)


def head_bwd(emb, params, out, g_out):
    e = emb.detach().clone().requires_grad_(True)
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    with torch.enable_grad():
        o = _head_chain(e, ps)
    return list(torch.autograd.grad(o, [e] + ps, g_out))


def knn_size_hint(min_nodes, max_nodes):
    """A performance hint of the kNN build (which kernel forms it runs): nothing to do for the oracle."""


def table_rowptr(nbr, cnt):
    N, k = nbr.shape
    valid = nbr >= 0
    if cnt is not None:
        valid = valid & (torch.arange(k).view(1, -1) < cnt.view(-1, 1))
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = valid.sum(1).cumsum(0).int()
    return rowptr


def table_edges(nbr, cnt, rowptr, num_edges, swap, want_index64, want_int32):
    N, k = nbr.shape
    slot = torch.arange(k).view(1, -1)
    inrow = slot < cnt.view(-1, 1) if cnt is not None else torch.ones((N, k), dtype=torch.bool)
    # as the kernel: a row that rowptr sizes at the full width k is copied slot for slot, -1 slots included
    verbatim = ((rowptr[1:] - rowptr[:-1]) == k).view(-1, 1)
    valid = inrow & ((nbr >= 0) | verbatim)
    assert int(valid.sum()) == num_edges == int(rowptr[-1]), "rowptr does not match the table"
    tgt = torch.arange(N, dtype=torch.int32).view(-1, 1).expand(N, k)[valid]
    src = nbr[valid]
    ei = None
    if want_index64:
        ei = torch.stack([tgt.long(), src.long()] if swap else [src.long(), tgt.long()], 0)
    return ei, (src.contiguous() if want_int32 else None), (tgt.contiguous() if want_int32 else None)


def table_order_by_count(cnt, ptr):
    """Per event: local node indices grouped by slot count, deepest rows first (any order inside a group)."""
    order = torch.empty(cnt.numel(), dtype=torch.int32)
    for b in range(ptr.numel() - 1):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        order[lo:hi] = torch.argsort(-cnt[lo:hi].long(), stable=True).int()
    return order


def gather_max_counted_j16(P, Q, nbr, cnt, order, ptr, sliced):
    """Counted gather that remembers the winner's event-local id (uint16 payload in an int16 tensor, 0xFFFF = none)."""
    if order is not None:   # a permutation of every event's local indices
        for b in range(ptr.numel() - 1):
            lo, hi = int(ptr[b]), int(ptr[b + 1])
            assert sorted(order[lo:hi].tolist()) == list(range(hi - lo))
    out, arg8 = gather_max(P, Q, nbr, ptr, True, cnt=cnt)
    N, H = out.shape
    counts = (ptr[1:] - ptr[:-1]).long()
    lo = torch.repeat_interleave(ptr[:-1], counts).view(-1, 1)
    slot = arg8.long().clamp(max=nbr.shape[1] - 1)
    j = torch.gather(nbr.long(), 1, slot) - lo
    j = torch.where(arg8 == 255, torch.full_like(j, 0xFFFF), j)
    return out, torch.where(j >= 0x8000, j - 0x10000, j).to(torch.int16)


def gather_max_local_j16(P, Q, rows16, cnt, order, ptr, kmax, sliced):
    """Rebuilds the int32 table from the uint16 rows (only slots < cnt are read) and runs the counted gather on it."""
    N = cnt.numel()
    counts = (ptr[1:] - ptr[:-1]).long()
    lo = torch.repeat_interleave(ptr[:-1], counts).view(-1, 1)
    ids = (rows16[:, :kmax].long() & 0xFFFF) + lo
    slot = torch.arange(kmax).view(1, -1)
    nbr = torch.where(slot < cnt.long().view(-1, 1), ids, torch.full_like(ids, 2 ** 30)).to(torch.int32)
    return gather_max_counted_j16(P, Q, nbr, cnt, order, ptr, sliced)


def gather_max_bwd_j16(g_out, argj, ptr, max_nodes=None, sliced=False):
    N, H = g_out.shape
    counts = (ptr[1:] - ptr[:-1]).long()
    lo = torch.repeat_interleave(ptr[:-1], counts).view(-1, 1)
    u = argj.long() & 0xFFFF
    valid = u != 0xFFFF
    j = u + lo
    gQ = torch.zeros_like(g_out)
    cols = torch.arange(H).expand(N, H)
    gQ.index_put_((j[valid], cols[valid]), g_out[valid], accumulate=True)
    return _to_sliced(gQ) if (sliced and H == 32) else gQ


_NAMES = ["knn_size_hint", "table_order_by_count", "gather_max_local_j16", "gather_max_counted_j16", "gather_max_bwd_j16", "table_rowptr", "table_edges", "head_fwd", "head_bwd", "met_loss", "gather_max_bwd_lds", "edgeconv_linear_bwd", "bn_fwd", "bn_bwd", "encode_fwd", "encode_bwd", "knn", "knn_local", "radius", "node_linear_split", "gather_max", "gather_max_bwd", "reverse_index", "edge_features",
          "edge_features_bwd", "segment_max", "segment_sum", "segment_max_bwd", "segment_sum_bwd", "met_reduce",
          "met_reduce_bwd", "segment_sum_1d", "batch_to_ptr", "xty", "onehot_xty", "edgeconv_fused_lds"]


def install(monkeypatch=None):
    """Replace deepmetv2_amd._native's entry points by the CPU stand-ins (for the duration of a test)."""
    import deepmetv2_amd._native as nat
    g = globals()
    for n in _NAMES:
        if monkeypatch is not None:
            monkeypatch.setattr(nat, n, g[n])
        else:
            setattr(nat, n, g[n])

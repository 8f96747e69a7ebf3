"""References for csrc/select.hip and deepmetv2_amd/select.py.

  * the ranking from its definition: plain Python sorted(range(n), key=(not isnan, -canonical score, index)) -- it knows
    nothing of the kernel's 64-bit key;
  * an emulation of that key (select_key) and the ranking it gives, held equal to the definition by the host tests;
  * restatements of filter_table, filter_edges, select_rows and its backward, in the dtype they are given (fp32: every
    output element is one multiply, so the kernels are held to its bits; float64: the reference of gs);
  * float64-capable restatements of upstream's published formulas for TopKPooling, SAGPooling (GraphConv scorer) and
    global_sort_pool, given the perm;
  * FakeKernels, which stands in for the five _native wrappers where the host logic is tested without a GPU.

gs bound: gs[i] = sum_f g[r,f] x[i,f] in fp32, any order, against float64 on the same fp32 operands: each product is
rounded once (u), then F - 1 additions: |err| <= gamma_F sum_f |g x|, gamma_n = n u / (1 - n u), u = 2^-24.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
T = 16384                          # DMET_SELECT_LDS_NODES
LENGTHS = [0, 0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4500, T - 1, T, T + 1, T + 3000, 0]
KINDS = ("gauss", "ties", "equal", "special")
RATIOS = (1.0, 0.5, 1e-4, 1, 30)
LAYER_LENGTHS = [0, 1, 2, 17, 64, 65, 130, 0, 257, 300]


def gamma(n):
    return n * U / (1 - n * U)


def ptr_of(lengths):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(lengths, dtype=torch.long).cumsum(0)])


def batch_of(lengths):
    return torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.0, -0.0, np.nan], dtype=np.float32)
NEG_NAN = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]


def scores(kind, lengths=None, seed=0):
    """score [N] fp32: 'gauss' N(0,1); 'ties' from {-1, 0, 1}; 'equal' all 0.25; 'special' a Gaussian seeded with +-0.0,
    +-inf, +NaN and -NaN (with payloads) at scattered positions of every event."""
    lengths = LENGTHS if lengths is None else lengths
    g = torch.Generator().manual_seed(500 + seed)
    N = sum(lengths)
    if kind == "gauss":
        return torch.randn(N, generator=g)
    if kind == "ties":
        return torch.randint(-1, 2, (N,), generator=g).float()
    if kind == "equal":
        return torch.full((N,), 0.25)
    x = torch.randn(N, generator=g).numpy().copy()
    pool = np.concatenate([SPECIALS, np.array([NEG_NAN], dtype=np.float32)])
    where = torch.randperm(N, generator=g)[: max(N // 3, min(N, 1))].numpy()
    x[where] = pool[np.arange(where.size) % pool.size]
    if N > 3:
        x[:3] = np.array([-0.0, 0.0, NEG_NAN], dtype=np.float32)
    return torch.from_numpy(x)


# ---- m_b ----------------------------------------------------------------------------------------------------------------------
def m_of(n, ratio):
    """Upstream's rule: ceil(fp32(n) * fp32(ratio)) for a float ratio, min(ratio, n) for an int."""
    if isinstance(ratio, int):
        return min(ratio, n)
    return int(math.ceil(float(np.float32(n) * np.float32(ratio))))


def slots_of(lengths, ratio):
    return [m_of(n, ratio) for n in lengths]


# ---- the ranking ----------------------------------------------------------------------------------------------------------------
def canonical(v):
    v = float(v)
    return 0.0 if v == 0.0 else v


def rank_event(vals):
    """Local indices of an event, best first: NaN first (above +inf), then descending canonical score, ties to the lower
    index."""
    vals = [float(v) for v in vals]
    return sorted(range(len(vals)), key=lambda i: (not math.isnan(vals[i]), -canonical(vals[i]) if not math.isnan(vals[i]) else 0.0, i))


def select_key(v, i):
    """The kernel's unsigned 64-bit key of local node i with fp32 score v."""
    u = int(np.array([v], dtype=np.float32).view(np.uint32)[0])
    if (u & 0x7FFFFFFF) > 0x7F800000:
        hi = 0xFFFFFFFF
    else:
        if u == 0x80000000:
            u = 0
        hi = (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)
    return (hi << 32) | (~i & 0xFFFFFFFF)


def rank_event_by_key(vals):
    keys = [select_key(v, i) for i, v in enumerate(vals)]
    assert len(set(keys)) == len(keys) and all(k > 0 for k in keys)
    return [(~k) & 0xFFFFFFFF for k in sorted(keys, reverse=True)]


_orders = {}


def orders_of(kind, lengths=None, seed=0):
    """The full ranking of every event of scores(kind, lengths, seed), computed once."""
    lengths = LENGTHS if lengths is None else lengths
    key = (kind, tuple(lengths), seed)
    if key not in _orders:
        s, ptr = scores(kind, lengths, seed).numpy(), ptr_of(lengths).tolist()
        _orders[key] = [rank_event(s[ptr[b]:ptr[b + 1]]) for b in range(len(lengths))]
    return _orders[key]


def topk(score, ptr, out_ptr, M, rank=rank_event, orders=None):
    """(perm[M] int64, node_map[N] int32) of dmet_topk_f32 from the definition (orders: the events' rankings when the
    caller has them already); slots no event owns stay -7."""
    s = score.detach().cpu().numpy().astype(np.float32)
    ptr, out_ptr = [int(v) for v in ptr.cpu().numpy()], [int(v) for v in out_ptr.cpu().numpy()]
    perm = np.full(M, -7, dtype=np.int64)
    node_map = np.full(s.size, -1, dtype=np.int32)
    for b in range(len(ptr) - 1):
        lo, n, o0 = ptr[b], ptr[b + 1] - ptr[b], out_ptr[b]
        r = min(out_ptr[b + 1] - o0, M - o0)
        order = orders[b] if orders is not None else rank(s[lo:lo + n])
        m = min(r, n)
        for p in range(m):
            perm[o0 + p] = lo + order[p]
            node_map[lo + order[p]] = o0 + p
        perm[o0 + m:o0 + max(r, m)] = -1
    return torch.from_numpy(perm), torch.from_numpy(node_map)


def topk_ratio(score, lengths, ratio, orders=None):
    """(perm, node_map, out_ptr) of topk(score, ratio) over a ragged batch."""
    out_ptr = ptr_of(slots_of(lengths, ratio))
    perm, node_map = topk(score, ptr_of(lengths), out_ptr, int(out_ptr[-1]), orders=orders)
    return perm, node_map, out_ptr


def min_score_perm(score, batch, B, min_score, tol=1e-7):
    smax = torch.full((B,), -float("inf"), dtype=score.dtype).scatter_reduce(0, batch, score, "amax", include_self=True)
    smin = (smax - tol).clamp(max=min_score)
    return (score > smin[batch]).nonzero().view(-1)


# ---- the operators --------------------------------------------------------------------------------------------------------------
def select_rows(x, s, perm):
    """out[r] = x[perm[r]] * s[perm[r]] in x's dtype (one rounding per element); perm < 0: zeros."""
    ok = perm >= 0
    p = perm.clamp(min=0)
    out = x[p] if s is None else x[p] * s[p].view(-1, 1)
    return torch.where(ok.view(-1, 1), out, torch.zeros_like(out))


def select_rows_bwd(g, x, s, node_map):
    """(gx, gs) in g's dtype; gs as a plain row sum (float64 operands: the reference; fp32: one of many orders)."""
    ok = (node_map >= 0).view(-1, 1)
    gr = g[node_map.clamp(min=0).long()] if g.shape[0] else g.new_zeros(node_map.numel(), g.shape[1])
    gx = gr if s is None else gr * s.view(-1, 1)
    gx = torch.where(ok, gx, torch.zeros_like(gx))
    prod = torch.where(ok, gr * x, torch.zeros_like(gr))
    return gx, prod.sum(1), prod.abs().sum(1)


def filter_table(nbr, cnt, perm, node_map):
    nbr_l, perm_l, nm = nbr.numpy().tolist(), perm.numpy().tolist(), node_map.numpy().tolist()
    N, k = nbr.shape
    out = np.full((len(perm_l), k), -1, dtype=np.int32)
    out_cnt = np.zeros(len(perm_l), dtype=np.int32)
    cnt_l = cnt.numpy().tolist() if cnt is not None else None
    for r, p in enumerate(perm_l):
        if p < 0:
            continue
        c = k if cnt_l is None else min(max(cnt_l[p], 0), k)
        kept = [nm[j] for j in nbr_l[p][:c] if 0 <= j < N and nm[j] >= 0]
        out[r, :len(kept)] = kept
        out_cnt[r] = len(kept)
    return torch.from_numpy(out), torch.from_numpy(out_cnt)


def filter_edges(edge_index, node_map):
    """(edge_index', kept, nbad): edges with both ends in range and picked, relabelled, in the caller's order."""
    N = node_map.numel()
    row, col = edge_index[0], edge_index[1]
    inr = (row >= 0) & (row < N) & (col >= 0) & (col < N)
    a = node_map[row.clamp(0, max(N - 1, 0))].long() if N else torch.full_like(row, -1)
    b = node_map[col.clamp(0, max(N - 1, 0))].long() if N else torch.full_like(col, -1)
    keep = inr & (a >= 0) & (b >= 0)
    kept = keep.nonzero().view(-1)
    return torch.stack([a[kept], b[kept]]), kept, int((~inr).sum())


# ---- upstream's layers, in the dtype of x, given the perm --------------------------------------------------------------------
def up_topk_score(x, w, act, batch=None, B=None, min_score=None):
    raw = (x * w).sum(-1)
    if min_score is None:
        return act(raw / w.norm(p=2, dim=-1))
    return up_softmax(raw, batch, B)


def up_softmax(src, batch, B):
    mx = torch.full((B,), -float("inf"), dtype=src.dtype).scatter_reduce(0, batch, src, "amax", include_self=True)
    e = (src - mx[batch]).exp()
    return e / torch.zeros(B, dtype=src.dtype).index_add(0, batch, e)[batch]


def up_graph_conv(x, edge_index, p):
    """GraphConv(in, 1): lin_rel(sum_j x_j) + lin_root(x_i) over edges j -> i (row 0 = source, row 1 = target)."""
    agg = torch.zeros_like(x).index_add(0, edge_index[1], x[edge_index[0]])
    return agg @ p["lin_rel.weight"].T + p["lin_rel.bias"] + x @ p["lin_root.weight"].T


def table_edges(nbr, cnt=None):
    """[2, E] of a table: row i lists the sources of target i; slot order."""
    N, k = nbr.shape
    slot = torch.arange(k).view(1, -1)
    ok = (nbr >= 0) & ((slot < cnt.view(-1, 1)) if cnt is not None else True)
    tgt = torch.arange(N).view(-1, 1).expand(N, k)
    return torch.stack([nbr[ok].long(), tgt[ok]])


def up_pool(x, score, perm, multiplier):
    """(x[perm] * score[perm] * multiplier, score[perm])."""
    out = x[perm] * score[perm].view(-1, 1)
    return (multiplier * out if multiplier != 1 else out), score[perm]


def up_sort_pool(x, lengths, k):
    """global_sort_pool: [B, k * F] in x's dtype."""
    F = x.shape[1]
    out = torch.zeros(len(lengths), k, F, dtype=x.dtype)
    lo = 0
    for b, n in enumerate(lengths):
        order = rank_event(x[lo:lo + n, -1].float().numpy())[:k]
        if order:
            out[b, :len(order)] = x[lo:lo + n][torch.tensor(order)]
        lo += n
    return out.view(len(lengths), k * F)


# ---- fakes ------------------------------------------------------------------------------------------------------------------------
class FakeKernels:
    """Stand-ins for deepmetv2_amd._native._topk / _select_rows / _select_rows_bwd / _filter_table / _filter_edges on CPU
    tensors, over the key emulation and the restatements above.  `calls` counts them by name."""

    def __init__(self):
        self.calls = {}

    def _note(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def topk(self, score, ptr, out_ptr, M):
        self._note("topk")
        assert score.dtype == torch.float32 and score.dim() == 1 and ptr.dtype == out_ptr.dtype == torch.int64
        perm, node_map = topk(score, ptr, out_ptr, int(M), rank=rank_event_by_key)
        assert int((perm == -7).sum()) == 0, "a slot of perm that no event owns"
        return perm, node_map

    def select_rows(self, x, s, perm):
        self._note("select_rows")
        assert x.dtype == torch.float32 and (s is None or s.dtype == torch.float32)
        return select_rows(x.detach(), None if s is None else s.detach(), perm)

    def select_rows_bwd(self, g, x, s, node_map, need_gx=True, need_gs=True):
        self._note("select_rows_bwd")
        gx, gs, _ = select_rows_bwd(g, x if x is not None else torch.zeros(node_map.numel(), g.shape[1]), s, node_map)
        return (gx if need_gx else None), (gs if need_gs else None)

    def filter_table(self, nbr, cnt, perm, node_map):
        self._note("filter_table")
        return filter_table(nbr, cnt, perm, node_map)

    def filter_edges(self, edge_index, node_map):
        self._note("filter_edges")
        out, kept, nbad = filter_edges(edge_index, node_map)
        return out, kept, torch.tensor([nbad], dtype=torch.int32)

    def install(self, monkeypatch):
        import deepmetv2_amd._native as nat
        for name in ("topk", "select_rows", "select_rows_bwd", "filter_table", "filter_edges"):
            monkeypatch.setattr(nat, "_" + name, getattr(self, name))
        return self

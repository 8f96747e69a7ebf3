"""float64 restatement of torch_geometric.nn.TransformerConv over a given graph, on the CPU, and the seeded inputs the
host and the GPU tests share.

PyG's forward is
    query = lin_query(x_dst).view(-1, H, C); key = lin_key(x_src).view(-1, H, C); value = lin_value(x_src).view(-1, H, C)
    alpha = softmax((query_i * key_j).sum(-1) / sqrt(C), index)          # utils.softmax: per target and head
    out   = sum_j alpha_ij value_j                                        # aggr = 'add'
    out   = out.view(-1, H * C) if concat else out.mean(1)
    x_r   = lin_skip(x_dst);  out = out + x_r,  or with beta: b = sigmoid(lin_beta([out, x_r, out - x_r])),
                                                              out = b x_r + (1 - b) out
The graph is a list of entries (tgt[E], src[E]); `table_entries` makes one from a fixed-width table whose slots hold -1
(or any id outside the source set) where they are empty.  The dtype follows the inputs, so the same code runs in
float32 for the check that the bars are reachable.
"""
import math

import torch


def table_entries(nbr, num_sources):
    """(tgt[E], src[E], pos[E]) of the valid slots of nbr[Nt, k] in position order, pos = i*k + t."""
    nbr = nbr.long()
    valid = (nbr >= 0) & (nbr < num_sources)
    i, t = valid.nonzero(as_tuple=True)
    return i, nbr[i, t], i * nbr.shape[1] + t


def attention(q, k, v, tgt, src):
    """(out[Nt, H, C], alpha[E, H], bar[Nt]) of q[Nt, H, C], k and v[Ns, H, C] over the entries src[e] -> tgt[e].
    Softmax by explicit max-subtraction per target and head; a target without an entry gives zeros.
    bar[i] = max over the row's entries of |v_j|_inf, the scale an output row's error is measured in."""
    Nt, H, C = q.shape
    tgt, src = tgt.long(), src.long()
    score = (q[tgt] * k[src]).sum(-1) / math.sqrt(C)
    ix = tgt.view(-1, 1).expand(-1, H)
    m = torch.full((Nt, H), float("-inf"), dtype=q.dtype).scatter_reduce(0, ix, score.detach(), "amax", include_self=True)
    p = torch.exp(score - m[tgt])
    l = torch.zeros((Nt, H), dtype=q.dtype).index_add(0, tgt, p)
    alpha = p / l[tgt]
    out = torch.zeros((Nt, H, C), dtype=q.dtype).index_add(0, tgt, alpha.unsqueeze(-1) * v[src])
    with torch.no_grad():
        vinf = v.abs().amax((1, 2)) if v.shape[0] else v.new_zeros(1)
        bar = torch.zeros(Nt, dtype=q.dtype).scatter_reduce(0, tgt, vinf[src], "amax", include_self=True)
    return out, alpha, bar


def g_q_term_scale(q, k, v, tgt, src, g):
    """max over the entries of |g_s_e| |k_j|_inf / sqrt(C) in float64, g_s_e = alpha_e (g_i . v_j - g_i . out_i): the
    size of the terms g_q[i,h,:] = sum_e g_s_e k[j,h,:] / sqrt(C) adds.  Where every k_j a row attends to is the same
    vector (equal scores; integer scores 32 apart, where only ties at the maximum carry weight) the exact sum is
    k sum_e g_s_e = 0 and max|g_q| is rounding noise, so g_q is held to 1e-4 of this scale instead: the rule
    tests/test_gpu_gravnet.py applies to lin_s.bias."""
    q, k, v, g = (t.detach().double() for t in (q, k, v, g))
    out, alpha, _bar = attention(q, k, v, tgt, src)
    tgt, src = tgt.long(), src.long()
    g_s = alpha * ((g[tgt] * v[src]).sum(-1) - (g * out).sum(-1)[tgt])
    return float((g_s.abs() * k[src].abs().amax(-1)).max()) / math.sqrt(q.shape[2]) if tgt.numel() else 0.0


def table_alpha(alpha, pos, num_rows, k):
    """alpha[E, H] of table_entries back in table form [Nt, k, H], zeros in the empty slots."""
    full = torch.zeros((num_rows * k, alpha.shape[1]), dtype=alpha.dtype)
    full[pos] = alpha
    return full.view(num_rows, k, -1)


class RefTransformerConv(torch.nn.Module):
    """The Linears of TransformerConv in float64 under PyG's names, applied over given entries."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, bias=True, root_weight=True):
        super().__init__()
        in_src, in_dst = (in_channels, in_channels) if isinstance(in_channels, int) else in_channels
        self.heads, self.out_channels, self.concat = heads, out_channels, concat
        self.lin_key = torch.nn.Linear(in_src, heads * out_channels).double()
        self.lin_query = torch.nn.Linear(in_dst, heads * out_channels).double()
        self.lin_value = torch.nn.Linear(in_src, heads * out_channels).double()
        width = heads * out_channels if concat else out_channels
        self.lin_skip = torch.nn.Linear(in_dst, width, bias=bias).double() if root_weight else None
        self.lin_beta = torch.nn.Linear(3 * width, 1, bias=False).double() if (beta and root_weight) else None

    def forward(self, x, tgt, src, return_alpha=False):
        x_src, x_dst = x if isinstance(x, (tuple, list)) else (x, x)
        H, C = self.heads, self.out_channels
        q = self.lin_query(x_dst).view(-1, H, C)
        k = self.lin_key(x_src).view(-1, H, C)
        v = self.lin_value(x_src).view(-1, H, C)
        self.key = k        # its .grad: the terms lin_key.bias's gradient sums
        if k.requires_grad:
            k.retain_grad()
        out, alpha, _bar = attention(q, k, v, tgt, src)
        out = out.reshape(-1, H * C) if self.concat else out.mean(1)
        if self.lin_skip is not None:
            x_r = self.lin_skip(x_dst)
            if self.lin_beta is not None:
                b = torch.sigmoid(self.lin_beta(torch.cat([out, x_r, out - x_r], -1)))
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        return (out, alpha) if return_alpha else out


# ---- the inputs of tests/test_gpu_attention.py, shared with the host test that shows its bars are reachable ---------------
# kNN tables: (event sizes, H, C, k)
KNN_CASES = {
    "short rows, a one-node and an empty event": ([1, 3, 0, 17, 40], 4, 16, 16),
    "smallest": ([5], 1, 1, 1),
    "limits": ([70, 64], 4, 64, 64),
    "two workgroups and more": ([300, 129, 7, 9, 19, 21, 31, 33], 2, 32, 20),
    "three chunks on 16 lanes": ([30, 34, 47], 3, 22, 33),
}
CHANNEL_WIDTHS = (1, 3, 4, 8, 15, 16, 17, 32, 33, 64)      # at H = 2, sizes [40, 9], k = 8
IN_DEGREES = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 600)


def qkv(num_targets, num_sources, H, C, seed):
    """q, k = 0.5 randn, v = randn: scores stay within a few units."""
    g = torch.Generator().manual_seed(seed)
    q = 0.5 * torch.randn(num_targets, H, C, generator=g)
    k = 0.5 * torch.randn(num_sources, H, C, generator=g)
    v = torch.randn(num_sources, H, C, generator=g)
    return q, k, v


def exact_score_inputs(num_nodes, H=2, seed=41):
    """C = 4, q = 16, k_j = m_j with integer m_j in [-3, 3]: scores 32 m_j, exact in fp32 and up to +-96 -- exp of them
    overflows fp32 unless the row's maximum is subtracted first."""
    g = torch.Generator().manual_seed(seed)
    q = torch.full((num_nodes, H, 4), 16.0)
    m = torch.randint(-3, 4, (num_nodes, H, 1), generator=g).float()
    return q, m.expand(-1, -1, 4).contiguous(), torch.randn(num_nodes, H, 4, generator=g)


def coords(num_nodes, seed):
    return torch.randn(num_nodes, 3, generator=torch.Generator().manual_seed(1000 + seed))


def host_knn(x, k, sizes):
    """nbr[N, k] int32 of the k nearest nodes of the same event, self included, -1 past a short event: the graph
    knn_table(x, k, batch, loop=True) builds (up to the order of equidistant neighbours), without a GPU."""
    N = x.shape[0]
    nbr = torch.full((N, k), -1, dtype=torch.int32)
    lo = 0
    for n in sizes:
        if n > 0:
            d = torch.cdist(x[lo:lo + n].double(), x[lo:lo + n].double())
            top = d.topk(min(k, n), dim=1, largest=False).indices
            nbr[lo:lo + n, :top.shape[1]] = (top + lo).to(torch.int32)
        lo += n
    return nbr


def degree_edge_index(seed=7):
    """int64 [2, E], shuffled: target t has IN_DEGREES[t] incoming edges (one of 600: a long row), source 0 is in every
    row of 600 further targets of in-degree 1 (a long reverse list), the other sources are drawn at random."""
    g = torch.Generator().manual_seed(seed)
    n_deg, hub = len(IN_DEGREES), 600
    N = n_deg + hub
    tgt = torch.cat([torch.full((d,), t, dtype=torch.int64) for t, d in enumerate(IN_DEGREES)]
                    + [torch.arange(n_deg, N, dtype=torch.int64)])
    src = torch.cat([torch.randint(1, N, (int(sum(IN_DEGREES)),), generator=g), torch.zeros(hub, dtype=torch.int64)])
    order = torch.randperm(tgt.numel(), generator=g)
    return torch.stack([src[order], tgt[order]]), N


# ---- the bars (tests/test_gpu_gravnet.py's), with `frac` for the host check that half of each is reachable in float32 -----------
def assert_output_bar(got, ref, bar, what="", frac=1.0):
    """Per row: |err| <= frac (1e-5 bar_i + 1e-6)."""
    got, ref = got.double().flatten(1), ref.double().flatten(1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.numel() == 0:
        return
    lim = frac * (1e-5 * bar.double() + 1e-6)
    err = (got - ref).abs().amax(1)
    assert bool((err <= lim).all()), (what, "out", float((err - lim).max()))


def assert_grad_bar(got, ref, what="", frac=1.0, scale=None):
    """rtol 1e-4, atol 1e-4 max|ref| (times frac).  scale: what stands in for max|ref| where the exact gradient is a sum
    that cancels to (nearly) zero -- the size of that sum's terms (g_q_term_scale)."""
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), (what, "not finite")
    scale = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6, scale or 0.0)
    torch.testing.assert_close(got, ref, rtol=frac * 1e-4, atol=frac * 1e-4 * scale, msg=lambda m: f"{what}: {m}")

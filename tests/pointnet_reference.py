"""float64 restatement of torch_geometric.nn.PointNetConv over a given graph, on the CPU, with an explicit backward and
a first-order fp32 rounding bound per value.

PyG's forward (aggr='max', flow source_to_target) is
    if add_self_loops: edge_index, _ = remove_self_loops(edge_index); edge_index, _ = add_self_loops(edge_index, N)
    msg_e = local_nn(torch.cat([x_j, pos_j - pos_i], dim=1))          j = edge_index[0, e], i = edge_index[1, e]
    out_i = max_e msg_e, zeros for a target without an edge;  then global_nn
Here local_nn = Linear(W1, b1) - act - Linear(W2, b2) [- act], act ReLU or ELU(alpha 1), and the graph is an ordered
entry list (tgt, src, code, is_self) grouped by target: the valid slots of a table row in slot order, or a grouped edge
list in position order, then -- with self loops -- one added entry i -> i (code -2, position difference exactly 0) after
the row's own, the written entries j == i having been dropped.  `code` is what the kernels' win holds for the entry: the
table slot or the list position.  Ties go to the earliest entry (R4).  The max is taken over the messages that are numbers
(nonfinite_contract.nan_skipping_max: a NaN never wins and never blocks); a channel of a target with entries whose
messages are all NaN is NaN with win -1.

Bounds.  u = 2^-24.  A value formed by a chain of fused multiply-adds s_k = fl(s_{k-1} + t_k) from s_0 carries, to first
order, at most u * sum_k |s_k| of rounding error: one rounding of magnitude at most u |s_k| per step.  The kernels form
    S = b1 + sum_f x W1x (f ascending),  P = sum_d pos W1p (d ascending),  A = fl(S + P),  pre1 = fl(A_j - P_i)
    z2 = b2 + sum_c h1_c W2[o, c] in the order c = 16 B + 4 q + t, B outermost, then t, then q (include/dmet.h)
so bar_pre1 sums |partial sums| of those chains plus |A| and |pre1| for the two extra roundings, bar_h1 = bar_pre1 (both
activations are 1-Lipschitz) + 4 u |h1| for expm1f, bar_z2 = sum_c |W2[o, c]| bar_h1[c] + u * (the chain's partial sums),
bar_m = bar_z2 + 4 u |m|.  An element is *fragile* when it lies within 8 x its bound of a ReLU kink (pre1, and z2 when
act2, under ReLU only: ELU with alpha 1 has no kink), or when the top two messages of a (target, channel) lie within 8 x
their summed bounds: there the winner, and so the routing of the gradient, may legitimately differ.  (Two messages that
a final ReLU clamped to exactly 0 are an exact tie everywhere and carry no gradient: not fragile.)
"""
import torch

U = 2.0 ** -24
F64 = torch.float64


def entries_from_table(nbr, num_sources, cnt=None, self_loop=False):
    """(tgt, src, code, is_self) int64 / bool, grouped by target in slot order; see the module text."""
    nbr = nbr.long()
    Nt, width = nbr.shape
    slot = torch.arange(width).view(1, -1).expand(Nt, width)
    row = torch.arange(Nt).view(-1, 1).expand(Nt, width)
    valid = (nbr >= 0) & (nbr < num_sources)
    if cnt is not None:
        valid &= slot < cnt.long().view(-1, 1)
    if self_loop:
        valid &= nbr != row
    tgt, src, code = row[valid], nbr[valid], slot[valid]
    return _append_self(tgt, src, code, Nt) if self_loop else (tgt, src, code, torch.zeros_like(tgt, dtype=torch.bool))


def entries_from_list(src, tgt, num_targets, self_loop=False):
    """The same for a list already grouped by target (tgt ascending): code = the position."""
    src, tgt = src.long(), tgt.long()
    code = torch.arange(src.numel())
    if self_loop:
        keep = src != tgt
        return _append_self(tgt[keep], src[keep], code[keep], num_targets)
    return tgt, src, code, torch.zeros_like(tgt, dtype=torch.bool)


def _append_self(tgt, src, code, N):
    ids = torch.arange(N)
    t = torch.cat([tgt, ids])
    order = torch.sort(t, stable=True).indices
    s = torch.cat([src, ids])[order]
    c = torch.cat([code, torch.full((N,), -2, dtype=torch.int64)])[order]
    f = torch.cat([torch.zeros_like(tgt, dtype=torch.bool), torch.ones(N, dtype=torch.bool)])[order]
    return t[order], s, c, f


def act_fn(v, act):
    return torch.where(v > 0, v, torch.expm1(v) if act == "elu" else torch.zeros_like(v))


def act_grad(v, act):
    """The derivative at pre-activation v (ReLU: 0 at and below 0; ELU: exp(v) below 0)."""
    return torch.where(v > 0, torch.ones_like(v), torch.exp(v) if act == "elu" else torch.zeros_like(v))


def _chain_bar(first, terms, order=None):
    """sum_k |s_k| of the chain s_0 = first, s_k = s_{k-1} + terms[..., order[k]] (s_0 is exact and not counted)."""
    if terms.shape[-1] == 0:
        return torch.zeros_like(first)
    if order is not None:
        terms = terms[..., order]
    return (first.unsqueeze(-1) + terms.cumsum(-1)).abs().sum(-1)


def mfma_order(H1):
    """The order in which dmet_pointnet_fwd_f32 adds the H1 products of z2: 16 B + 4 q + t, B, then t, then q."""
    ks = [16 * B + 4 * q + t for B in range((H1 + 15) // 16) for t in range(4) for q in range(4)]
    return torch.tensor([k for k in ks if k < H1], dtype=torch.int64)


class Reference:
    """Everything of one forward: out, win (entry code, -1 none), the fragile count and, through backward(g), the
    gradients.  All float64 CPU tensors; x may be None (F = 0); b1 / b2 may be None."""

    def __init__(self, x, pos_src, pos_dst, W1, b1, W2, b2, act, act2, entries, num_targets):
        from nonfinite_contract import nan_skipping_max
        tgt, src, code, is_self = entries
        d = lambda t: None if t is None else t.detach().cpu().to(F64)
        x, pos_src, pos_dst, W1, b1, W2, b2 = map(d, (x, pos_src, pos_dst, W1, b1, W2, b2))
        Ns, D = pos_src.shape
        F = 0 if x is None else x.shape[1]
        H1, H2 = W1.shape[0], W2.shape[0]
        if x is None:
            x = pos_src.new_zeros((Ns, 0))
        b1 = W1.new_zeros(H1) if b1 is None else b1
        b2 = W2.new_zeros(H2) if b2 is None else b2
        self.args = (x, pos_src, pos_dst, W1, W2)
        self.act, self.act2, self.Nt, self.F = act, act2, num_targets, F
        self.tgt, self.src, self.code, self.is_self = tgt, src, code, is_self
        E = tgt.numel()
        diff = pos_src[src] - pos_dst[tgt]
        diff[is_self] = 0.0
        self.feat = torch.cat([x[src], diff], dim=1)                            # [E, F + D]
        self.pre1 = self.feat @ W1.t() + b1
        self.h1 = act_fn(self.pre1, act)
        self.z2 = self.h1 @ W2.t() + b2
        self.m = act_fn(self.z2, act) if act2 else self.z2
        # ---- bounds -------------------------------------------------------------------------------------------------
        W1x, W1p = W1[:, :F], W1[:, F:]
        s_terms = x.unsqueeze(1) * W1x.unsqueeze(0)                             # [Ns, H1, F]
        S = b1 + s_terms.sum(-1)
        bar_S = _chain_bar(b1.expand(Ns, H1), s_terms)
        ps_terms = pos_src.unsqueeze(1) * W1p.unsqueeze(0)
        pd_terms = pos_dst.unsqueeze(1) * W1p.unsqueeze(0)
        Ps, Pd = ps_terms.sum(-1), pd_terms.sum(-1)
        bar_Ps = _chain_bar(torch.zeros(Ns, H1, dtype=F64), ps_terms)
        bar_Pd = _chain_bar(torch.zeros(pos_dst.shape[0], H1, dtype=F64), pd_terms)
        bar_A = bar_S + bar_Ps + (S + Ps).abs()
        bar_pre1 = torch.where(is_self.view(-1, 1), bar_S[src], bar_A[src] + bar_Pd[tgt] + self.pre1.abs()) * U
        bar_h1 = bar_pre1 + 4 * U * self.h1.abs()
        z_terms = self.h1.unsqueeze(1) * W2.unsqueeze(0)                        # [E, H2, H1]
        bar_z2 = bar_h1 @ W2.abs().t() + U * _chain_bar(b2.expand(E, H2), z_terms, mfma_order(H1))
        self.bar_m = bar_z2 + 4 * U * self.m.abs()
        # ---- max, ties to the earliest entry --------------------------------------------------------------------------
        self.out = torch.zeros((num_targets, H2), dtype=F64)
        self.win_e = torch.full((num_targets, H2), -1, dtype=torch.int64)     # index into the entry list
        self.win = torch.full((num_targets, H2), -1, dtype=torch.int64)       # the entry's code
        fragile = 0
        if act == "relu":
            fragile += int((self.pre1.abs() <= 8 * bar_pre1).sum())
            if act2:
                fragile += int((self.z2.abs() <= 8 * bar_z2).sum())
        rowptr = torch.zeros(num_targets + 1, dtype=torch.int64)
        rowptr[1:] = torch.bincount(tgt, minlength=num_targets).cumsum(0)
        self.rowptr = rowptr
        for i in range(num_targets):
            lo, hi = int(rowptr[i]), int(rowptr[i + 1])
            if hi == lo:
                continue
            mi = self.m[lo:hi]
            top, first = nan_skipping_max(mi.t(), torch.ones(H2, hi - lo, dtype=torch.bool))   # the earliest entry holding it
            self.out[i] = top
            self.win_e[i] = torch.where(first >= 0, lo + first, first)
            self.win[i] = torch.where(first >= 0, code[lo + first.clamp(min=0)], first)
            first = first.clamp(min=0)
            if hi - lo > 1:
                cols = torch.arange(H2)
                rest = mi.clone()
                rest[first, cols] = -float("inf")
                second = rest.argmax(0)
                gap = top - rest[second, cols]
                lim = 8 * (self.bar_m[lo + first, cols] + self.bar_m[lo + second, cols])
                # two messages a final ReLU clamped to exactly 0 tie exactly on every machine (their z2 are clear of the
                # kink, or counted above): the earliest wins by R4 and no gradient passes either
                clamped = (top == 0) & (rest[second, cols] == 0) if (act2 and act == "relu") else torch.zeros_like(top, dtype=torch.bool)
                fragile += int(((gap <= lim) & ~clamped).sum())
        self.fragile = fragile

    def backward(self, g):
        """{name: gradient} for g = d loss / d out [Nt, H2]: x, pos_src, pos_dst, W1, b1, W2, b2."""
        x, pos_src, pos_dst, W1, W2 = self.args
        g = g.detach().cpu().to(F64)
        F, E, H2 = self.F, self.tgt.numel(), W2.shape[0]
        gz = torch.zeros((E, H2), dtype=F64)
        has = self.win_e >= 0
        ii, oo = has.nonzero(as_tuple=True)
        ee = self.win_e[ii, oo]
        gm = g[ii, oo]
        if self.act2:
            gm = gm * act_grad(self.z2[ee, oo], self.act)
        gz[ee, oo] = gm
        g_h1 = gz @ W2
        g_pre1 = g_h1 * act_grad(self.pre1, self.act)
        g_feat = g_pre1 @ W1
        gx = torch.zeros_like(x).index_add_(0, self.src, g_feat[:, :F])
        gpos = g_feat[:, F:].clone()
        gpos[self.is_self] = 0.0                                               # the added entry reads no position
        gps = torch.zeros_like(pos_src).index_add_(0, self.src, gpos)
        gpd = torch.zeros_like(pos_dst).index_add_(0, self.tgt, -gpos)
        return {"x": gx, "pos_src": gps, "pos_dst": gpd, "W1": g_pre1.t() @ self.feat, "b1": g_pre1.sum(0),
                "W2": gz.t() @ self.h1, "b2": gz.sum(0)}

    def listed(self):
        """bool [Ns]: the sources some entry (the added self entry included) names."""
        m = torch.zeros(self.args[1].shape[0], dtype=torch.bool)
        m[self.src] = True
        return m


def loops(x, pos_src, pos_dst, W1, b1, W2, b2, act, act2, entries, num_targets):
    """The forward as a plain triple loop over targets, entries and channels, in Python floats: (out, win code)."""
    import math
    tgt, src, code, is_self = [t.tolist() for t in entries]
    H1, H2 = W1.shape[0], W2.shape[0]
    F = 0 if x is None else x.shape[1]
    D = pos_src.shape[1]
    f = lambda v: v if v > 0 else (math.expm1(v) if act == "elu" else 0.0)
    out = [[0.0] * H2 for _ in range(num_targets)]
    win = [[-1] * H2 for _ in range(num_targets)]
    for e in range(len(tgt)):
        i, j = tgt[e], src[e]
        feat = [float(x[j, k]) for k in range(F)] + [0.0 if is_self[e] else float(pos_src[j, k]) - float(pos_dst[i, k])
                                                     for k in range(D)]
        h1 = [f((float(b1[c]) if b1 is not None else 0.0) + sum(float(W1[c, k]) * feat[k] for k in range(F + D)))
              for c in range(H1)]
        for o in range(H2):
            z = (float(b2[o]) if b2 is not None else 0.0) + sum(float(W2[o, c]) * h1[c] for c in range(H1))
            m = f(z) if act2 else z
            if win[i][o] == -1 or m > out[i][o]:
                out[i][o], win[i][o] = m, code[e]
    return torch.tensor(out, dtype=F64).view(num_targets, H2), torch.tensor(win, dtype=torch.int64).view(num_targets, H2)

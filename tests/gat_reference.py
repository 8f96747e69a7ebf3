"""float64 restatement of torch_geometric.nn.GATv2Conv and torch_geometric.nn.GATConv over a given graph, on the CPU,
and the seeded inputs the host and the GPU tests share.

PyG's GATv2Conv forward is
    x_l = lin_l(x_src).view(-1, H, C); x_r = lin_r(x_dst).view(-1, H, C)          # lin_r is lin_l with share_weights
    edge_index = add_self_loops(remove_self_loops(edge_index))                     # add_self_loops=True
    alpha = softmax((F.leaky_relu(x_l[j] + x_r[i], negative_slope) * att).sum(-1), index)   # per target and head
    out   = sum_j alpha_ij x_l[j]                                                   # aggr = 'add'
    out   = out.view(-1, H * C) if concat else out.mean(1);  out = out + res(x_dst);  out = out + bias
and GATConv's differs in the score:
    x_l = lin(x_src) (lin_src), x_d = lin(x_dst) (lin_dst)
    alpha = softmax(F.leaky_relu((x_l * att_src).sum(-1)[j] + (x_d * att_dst).sum(-1)[i], negative_slope), index)
The graph is a list of entries (tgt[E], src[E]); `with_self_loops` is the rewrite add_self_loops=True stands for.  The
dtype follows the inputs, so the same code runs in float32 for the check that the bars are reachable.  utils.softmax adds
1e-16 to its denominator, which is at least 1: it is left out here as in the kernels, and float64 cannot tell.
"""
import math

import torch
import torch.nn.functional as F

import attention_reference as ar
from attention_reference import (CHANNEL_WIDTHS, IN_DEGREES, KNN_CASES, assert_grad_bar, assert_output_bar,  # noqa: F401
                                 degree_edge_index, table_alpha, table_entries)

V1, V2 = 1, 2


def with_self_loops(tgt, src, num_nodes):
    """remove_self_loops + add_self_loops: the entries with src != tgt in their order, then i -> i for every node."""
    tgt, src = tgt.long(), src.long()
    keep = tgt != src
    loop = torch.arange(num_nodes, dtype=torch.int64)
    return torch.cat([tgt[keep], loop]), torch.cat([src[keep], loop])


def _softmax_sum(score, xl, tgt, src, num_targets):
    """(out[Nt, H, C], alpha[E, H], bar[Nt]) of the scores score[E, H] over the entries src[e] -> tgt[e]; softmax by
    explicit max-subtraction per target and head; a target without an entry gives zeros.  bar[i] = max over the row's
    entries of |xl_j|_inf, the scale an output row's error is measured in."""
    H, C = xl.shape[1], xl.shape[2]
    ix = tgt.view(-1, 1).expand(-1, H)
    m = torch.full((num_targets, H), float("-inf"), dtype=xl.dtype).scatter_reduce(0, ix, score.detach(), "amax",
                                                                                    include_self=True)
    p = torch.exp(score - m[tgt])
    l = torch.zeros((num_targets, H), dtype=xl.dtype).index_add(0, tgt, p)
    alpha = p / l[tgt]
    out = torch.zeros((num_targets, H, C), dtype=xl.dtype).index_add(0, tgt, alpha.unsqueeze(-1) * xl[src])
    with torch.no_grad():
        xinf = xl.abs().amax((1, 2)) if xl.shape[0] else xl.new_zeros(1)
        bar = torch.zeros(num_targets, dtype=xl.dtype).scatter_reduce(0, tgt, xinf[src], "amax", include_self=True)
    return out, alpha, bar


def gatv2(xl, xr, att, tgt, src, slope):
    """(out, alpha, bar) of GATv2's attention: xl[Ns, H, C], xr[Nt, H, C], att[H, C]."""
    tgt, src = tgt.long(), src.long()
    score = (F.leaky_relu(xl[src] + xr[tgt], slope) * att.reshape(1, xl.shape[1], xl.shape[2])).sum(-1)
    return _softmax_sum(score, xl, tgt, src, xr.shape[0])


def gatv1(xl, s_src, s_dst, tgt, src, slope):
    """(out, alpha, bar) of GAT's attention: xl[Ns, H, C], s_src[Ns, H], s_dst[Nt, H]."""
    tgt, src = tgt.long(), src.long()
    score = F.leaky_relu(s_src[src] + s_dst[tgt], slope)
    return _softmax_sum(score, xl, tgt, src, s_dst.shape[0])


def run(mode, xl, a, b, tgt, src, slope):
    return gatv2(xl, a, b, tgt, src, slope) if mode == V2 else gatv1(xl, a, b, tgt, src, slope)


def term_scale(mode, xl, a, b, tgt, src, slope, g):
    """max over the entries (and channels) of |d_e| in float64, d_e the term the target-side gradient sums over a row:
    v2, g_xr[i,h,c] = sum_e g_s_e att[h,c] lrelu'(t_e[c]); v1, g_s_dst[i,h] = sum_e g_s_e lrelu'(t_e);
    g_s_e = alpha_e (g_i . xl_j - g_i . out_i).  Where every t_e of a row lies on one side of 0 (or slope == 1) lrelu' is
    one constant, the exact sum is that constant times sum_e g_s_e = 0, and max|ref| is rounding noise; the gradient is
    then held to 1e-4 of this scale instead, the rule attention_reference.g_q_term_scale applies to g_q."""
    xl, a, b, g = (t.detach().double() for t in (xl, a, b, g))
    tgt, src = tgt.long(), src.long()
    if tgt.numel() == 0:
        return 0.0
    out, alpha, _bar = run(mode, xl, a, b, tgt, src, slope)
    g_s = alpha * ((g[tgt] * xl[src]).sum(-1) - (g * out).sum(-1)[tgt])
    if mode == V2:
        t = xl[src] + a[tgt]
        d = g_s.unsqueeze(-1) * b.reshape(1, xl.shape[1], xl.shape[2]) * torch.where(t > 0, 1.0, float(slope))
    else:
        t = a[src] + b[tgt]
        d = g_s * torch.where(t > 0, 1.0, float(slope))
    return float(d.abs().max())


def _glorot_(t, gen):
    a = math.sqrt(6.0 / (t.shape[-2] + t.shape[-1]))
    with torch.no_grad():
        t.copy_((torch.rand(t.shape, generator=gen, dtype=torch.float64) * 2 - 1) * a)


class _RefBase(torch.nn.Module):
    def _tail(self, in_dst, heads, out_channels, concat, bias, residual, gen):
        width = heads * out_channels if concat else out_channels
        self.heads, self.out_channels, self.concat = heads, out_channels, concat
        self.res = torch.nn.Linear(in_dst, width, bias=False).double() if residual else None
        if bias:
            self.bias = torch.nn.Parameter(torch.rand(width, generator=gen, dtype=torch.float64) - 0.5)
        else:
            self.register_parameter("bias", None)

    def _finish(self, out, x_dst):
        out = out.reshape(-1, self.heads * self.out_channels) if self.concat else out.mean(1)
        if self.res is not None:
            out = out + self.res(x_dst)
        if self.bias is not None:
            out = out + self.bias
        return out


class RefGATv2Conv(_RefBase):
    """GATv2Conv in float64 under PyG's parameter names, applied over given entries.  The bias starts non-zero so that a
    loaded state shows in the output."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True,
                 share_weights=False, residual=False, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        in_src, in_dst = (in_channels, in_channels) if isinstance(in_channels, int) else in_channels
        self.negative_slope, self.share_weights = negative_slope, share_weights
        self.lin_l = torch.nn.Linear(in_src, heads * out_channels).double()
        self.lin_r = self.lin_l if share_weights else torch.nn.Linear(in_dst, heads * out_channels).double()
        self.att = torch.nn.Parameter(torch.empty(1, heads, out_channels, dtype=torch.float64))
        _glorot_(self.att, gen)
        self._tail(in_dst, heads, out_channels, concat, bias, residual, gen)

    def forward(self, x, tgt, src, add_self_loops=False, return_alpha=False):
        x_src, x_dst = x if isinstance(x, (tuple, list)) else (x, x)
        H, C = self.heads, self.out_channels
        xl = self.lin_l(x_src).view(-1, H, C)
        xr = self.lin_r(x_dst).view(-1, H, C)
        if add_self_loops:
            tgt, src = with_self_loops(tgt, src, x_dst.shape[0])
        out, alpha, _bar = gatv2(xl, xr, self.att, tgt, src, self.negative_slope)
        out = self._finish(out, x_dst)
        return (out, alpha) if return_alpha else out


class RefGATConv(_RefBase):
    """GATConv in float64 under PyG's parameter names, applied over given entries."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True, residual=False,
                 seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.negative_slope = negative_slope
        if isinstance(in_channels, int):
            self.lin = torch.nn.Linear(in_channels, heads * out_channels, bias=False).double()
            self.lin_src = self.lin_dst = None
            in_dst = in_channels
        else:
            self.lin = None
            self.lin_src = torch.nn.Linear(in_channels[0], heads * out_channels, bias=False).double()
            self.lin_dst = torch.nn.Linear(in_channels[1], heads * out_channels, bias=False).double()
            in_dst = in_channels[1]
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels, dtype=torch.float64))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels, dtype=torch.float64))
        _glorot_(self.att_src, gen)
        _glorot_(self.att_dst, gen)
        self._tail(in_dst, heads, out_channels, concat, bias, residual, gen)

    def forward(self, x, tgt, src, add_self_loops=False, return_alpha=False):
        x_src, x_dst = x if isinstance(x, (tuple, list)) else (x, x)
        H, C = self.heads, self.out_channels
        lin_src, lin_dst = (self.lin, self.lin) if self.lin is not None else (self.lin_src, self.lin_dst)
        xl = lin_src(x_src).view(-1, H, C)
        xd = lin_dst(x_dst).view(-1, H, C)
        if add_self_loops:
            tgt, src = with_self_loops(tgt, src, x_dst.shape[0])
        out, alpha, _bar = gatv1(xl, (xl * self.att_src).sum(-1), (xd * self.att_dst).sum(-1), tgt, src, self.negative_slope)
        out = self._finish(out, x_dst)
        return (out, alpha) if return_alpha else out


# ---- the inputs of tests/test_gpu_gat.py, shared with the host test that shows its bars are reachable -----------------------
KINDS = ("random", "positive", "negative", "zeros", "large")


def inputs(mode, num_targets, num_sources, H, C, seed, kind="random"):
    """(xl[Ns, H, C], a, b) fp32 on the CPU; (a, b) = (xr[Nt, H, C], att[H, C]) for V2, (s_src[Ns, H], s_dst[Nt, H]) for V1.
    random: scores within a few units.  positive / negative: every xl + xr (s_src + s_dst) on one side of 0.  zeros:
    integers in {-1, 0, 1}, so many sums are exactly 0.  large (C >= 8, slope 0.5): integer-valued score operands, scores
    exact in fp32 and up to +-100 or so -- exp of them overflows fp32 unless the row's maximum is subtracted first; for V2
    att is 8 on the first four channels and 0 beyond, where xl carries the random values the output mixes."""
    g = torch.Generator().manual_seed(seed)
    Nt, Ns = num_targets, num_sources

    def signed(shape):
        base = 0.1 + torch.rand(shape, generator=g)
        return base if kind == "positive" else -base

    if kind == "large":
        assert C >= 8
        m = torch.randint(-3, 4, (Ns, H, 1), generator=g).float()
        r = torch.randint(-1, 2, (Nt, H, 1), generator=g).float()
        xl = torch.randn(Ns, H, C, generator=g)
        if mode == V1:
            return xl, 32.0 * m[:, :, 0], 8.0 * r[:, :, 0]
        xl[:, :, :4] = m
        xr = torch.randn(Nt, H, C, generator=g)
        xr[:, :, :4] = r
        att = torch.zeros(H, C)
        att[:, :4] = 8.0
        return xl, xr, att
    if mode == V2:
        att = torch.randn(H, C, generator=g) / math.sqrt(C)
        if kind == "random":
            return torch.randn(Ns, H, C, generator=g), 0.5 * torch.randn(Nt, H, C, generator=g), att
        if kind == "zeros":
            return (torch.randint(-1, 2, (Ns, H, C), generator=g).float(),
                    torch.randint(-1, 2, (Nt, H, C), generator=g).float(), att)
        return signed((Ns, H, C)), signed((Nt, H, C)), att
    xl = torch.randn(Ns, H, C, generator=g)
    if kind == "random":
        return xl, torch.randn(Ns, H, generator=g), torch.randn(Nt, H, generator=g)
    if kind == "zeros":
        return xl, torch.randint(-1, 2, (Ns, H), generator=g).float(), torch.randint(-1, 2, (Nt, H), generator=g).float()
    return xl, signed((Ns, H)), signed((Nt, H))


def loops_edge_index(seed=11):
    """int64 [2, E], shuffled, over 50 nodes: random edges, a written self loop on every third node (two on node 3), node 49
    isolated (no edge at all) and node 48 with nothing but its own written loop."""
    g = torch.Generator().manual_seed(seed)
    N, E = 50, 300
    src = torch.randint(0, 48, (E,), generator=g)
    tgt = torch.randint(0, 48, (E,), generator=g)
    loops = torch.cat([torch.arange(0, 48, 3), torch.tensor([3, 48])])
    src, tgt = torch.cat([src, loops]), torch.cat([tgt, loops])
    order = torch.randperm(src.numel(), generator=g)
    return torch.stack([src[order], tgt[order]]), N


# name -> graph ("knn", sizes, k, loop) | ("degree",) | ("loops",), H, C, seed, kind, slope, self_loops
OPERATOR_CASES = {}
for _name, (_sizes, _H, _C, _k) in KNN_CASES.items():
    OPERATOR_CASES["knn, " + _name] = dict(graph=("knn", _sizes, _k, True), H=_H, C=_C, seed=len(_name))
for _C in CHANNEL_WIDTHS:
    OPERATOR_CASES[f"width C={_C}"] = dict(graph=("knn", [40, 9], 8, True), H=2, C=_C, seed=_C)
for _H, _C in ((2, 16), (1, 40)):
    OPERATOR_CASES[f"in-degrees H={_H} C={_C}"] = dict(graph=("degree",), H=_H, C=_C, seed=31)
OPERATOR_CASES["self loops over knn_table(loop=False)"] = dict(graph=("knn", [30, 1, 12], 8, False), H=2, C=16, seed=81,
                                                               self_loops=True)
OPERATOR_CASES["self loops over a list with written loops"] = dict(graph=("loops",), H=3, C=22, seed=82, self_loops=True)
OPERATOR_CASES["self loops over the in-degrees"] = dict(graph=("degree",), H=1, C=40, seed=83, self_loops=True)
for _kind in ("positive", "negative", "zeros"):
    OPERATOR_CASES[f"lrelu {_kind}"] = dict(graph=("knn", [40, 9], 8, True), H=2, C=20, seed=84, kind=_kind)
OPERATOR_CASES["lrelu slope 0"] = dict(graph=("knn", [40, 9], 8, True), H=2, C=20, seed=85, slope=0.0)
OPERATOR_CASES["lrelu slope 1"] = dict(graph=("knn", [40, 9], 8, True), H=2, C=20, seed=86, slope=1.0)
OPERATOR_CASES["lrelu zeros, slope 0"] = dict(graph=("knn", [40, 9], 8, True), H=2, C=20, seed=87, kind="zeros", slope=0.0)
OPERATOR_CASES["large scores"] = dict(graph=("degree",), H=2, C=8, seed=88, kind="large", slope=0.5)
OPERATOR_CASES["large scores, self loops"] = dict(graph=("loops",), H=2, C=8, seed=89, kind="large", slope=0.5,
                                                  self_loops=True)
for _case in OPERATOR_CASES.values():
    _case.setdefault("kind", "random")
    _case.setdefault("slope", 0.2)
    _case.setdefault("self_loops", False)


def cancelling(case):
    """The target-side gradient (g_xr / g_s_dst) of this case is a sum that cancels exactly in every row: one sign of
    xl + xr, a slope of 1, or (large) integer scores 8 or more apart, where only ties at the maximum carry weight and tied
    entries hold the same operands."""
    return case["kind"] in ("positive", "negative", "large") or case["slope"] == 1.0


def case_nodes(case):
    g = case["graph"]
    if g[0] == "knn":
        return sum(g[1])
    return degree_edge_index()[1] if g[0] == "degree" else loops_edge_index()[1]


def host_entries(case):
    """(tgt, src, N) of a case's graph as written (before the self-loop rewrite), built without a GPU."""
    g = case["graph"]
    if g[0] == "knn":
        _kind, sizes, k, loop = g
        N = sum(sizes)
        x = ar.coords(N, case["seed"])
        if loop:
            nbr = ar.host_knn(x, k, sizes)
        else:       # the k nearest others: the self column of k + 1 dropped
            wide = ar.host_knn(x, k + 1, sizes)
            me = torch.arange(N, dtype=torch.int32).view(-1, 1)
            nbr = torch.full((N, k), -1, dtype=torch.int32)
            for i in range(N):
                row = wide[i][(wide[i] != me[i]) & (wide[i] >= 0)][:k]
                nbr[i, :row.numel()] = row
        tgt, src, _pos = table_entries(nbr, N)
        return tgt, src, N
    ei, N = degree_edge_index() if g[0] == "degree" else loops_edge_index()
    return ei[1], ei[0], N


# the modules: name -> (class, in_channels, constructor options); heads 3, out_channels 6
MODULE_CASES = {
    "v2 concat, self loops": ("v2", 10, dict(concat=True, add_self_loops=True)),
    "v2 mean, shared, residual": ("v2", 10, dict(concat=False, share_weights=True, residual=True, add_self_loops=True)),
    "v2 no bias, no loops": ("v2", 10, dict(bias=False, add_self_loops=False)),
    "v2 pair": ("v2", (7, 9), dict(add_self_loops=False, residual=True)),
    "v1 concat, self loops": ("v1", 10, dict(concat=True, add_self_loops=True)),
    "v1 mean, residual": ("v1", 10, dict(concat=False, residual=True, add_self_loops=True)),
    "v1 no bias, no loops": ("v1", 10, dict(bias=False, add_self_loops=False)),
    "v1 pair": ("v1", (7, 9), dict(add_self_loops=False, residual=True, negative_slope=0.3)),
}


def module_inputs(name):
    """(x or (x_src, x_dst), edge_index int64 [2, E] shuffled with written self loops, num_src, num_dst) of a module case."""
    _cls, in_channels, _opts = MODULE_CASES[name]
    g = torch.Generator().manual_seed(len(name) + 90)
    if isinstance(in_channels, int):
        N, E = 57, 400
        x = torch.randn(N, in_channels, generator=g)
        ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N - 3, (E,), generator=g)])
        return x, ei, N, N
    ns, nd = 23, 35
    x = (torch.randn(ns, in_channels[0], generator=g), torch.randn(nd, in_channels[1], generator=g))
    ei = torch.stack([torch.randint(0, ns, (300,), generator=g), torch.randint(0, nd - 2, (300,), generator=g)])
    return x, ei, ns, nd


def ref_module(name, seed=0):
    cls, in_channels, opts = MODULE_CASES[name]
    opts = {k: v for k, v in opts.items() if k != "add_self_loops"}
    torch.manual_seed(seed + 7)
    return (RefGATv2Conv if cls == "v2" else RefGATConv)(in_channels, 6, heads=3, seed=seed, **opts)

"""Float64 restatements for csrc/weighted_sum.hip, deepmetv2_amd/propagate.py and deepmetv2_amd/gcn.py, the error bounds the
GPU tests hold the kernels to, an fp32 numpy emulation of the kernels' own chains (for the host tests: it must stay under
half of every bound, and it stands in for the kernels where the layers' host logic is tested without a GPU), and PyG's
GCNConv / GraphConv / SAGEConv / GINConv composed per edge as their published source composes them.

A graph is given as positions, as in tests/pna_reference.py: tgt[P], src[P] and valid[P] in ascending position order.

Bounds, u = 2^-24, against float64 on the same fp32 inputs (the issue's):
  out     (n_i + 2) u sum_e |w_e x[j_e,f]|        one rounding per fma, n_i terms
  g_x     (n_j + 2) u sum_p |w_p g_out[i,f]|      the same chain by source
  g_w[p]  (F + 8) u sum_f |g_out[i,f] x[j,f]|     one product rounding, then additions: a lane owns four consecutive
                                                  features and adds them in order from 0 (at most 3 inexact additions,
                                                  0 + p is exact), then log2(lanes) <= 6 butterfly additions, of which
                                                  those that add the 0 of an idle lane are exact: a product passes
                                                  through at most 1 + min(F, 4) - 1 + ceil(log2(ceil(F / 4))) <= 10
                                                  roundings, never more than F + 8
  empty rows, unlisted sources, empty slots: exactly 0;  count: equal.
"""
import numpy as np
import torch

from pna_reference import positions_of_list, positions_of_table  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24


# ---- float64 ---------------------------------------------------------------------------------------------------------------
def _valid(tgt, src, valid):
    pos = torch.nonzero(valid).view(-1)
    return pos, tgt[pos], src[pos]


def forward(x, w, tgt, src, valid, Nt):
    """(out [Nt, F], count [Nt], bound [Nt, F]) in float64; w [P] or None."""
    x = x.double()
    pos, i, j = _valid(tgt, src, valid)
    wv = torch.ones(pos.numel(), dtype=torch.float64) if w is None else w.double().reshape(-1)[pos]
    term = wv.view(-1, 1) * x[j]
    out = torch.zeros(Nt, x.shape[1], dtype=torch.float64).index_add_(0, i, term)
    mag = torch.zeros_like(out).index_add_(0, i, term.abs())
    count = torch.bincount(i, minlength=Nt)
    return out, count, (count.double().view(-1, 1) + 2) * U * mag


def grad_x(g_out, w, tgt, src, valid, Ns):
    """(g_x [Ns, F], n_j [Ns], bound [Ns, F]) in float64."""
    g = g_out.double()
    pos, i, j = _valid(tgt, src, valid)
    wv = torch.ones(pos.numel(), dtype=torch.float64) if w is None else w.double().reshape(-1)[pos]
    term = wv.view(-1, 1) * g[i]
    g_x = torch.zeros(Ns, g.shape[1], dtype=torch.float64).index_add_(0, j, term)
    mag = torch.zeros_like(g_x).index_add_(0, j, term.abs())
    n_j = torch.bincount(j, minlength=Ns)
    return g_x, n_j, (n_j.double().view(-1, 1) + 2) * U * mag


def grad_w(g_out, x, tgt, src, valid):
    """(g_w [P], bound [P]) in float64; 0 at every position that is no entry."""
    g, x = g_out.double(), x.double()
    F = x.shape[1]
    pos, i, j = _valid(tgt, src, valid)
    prod = g[i] * x[j]
    g_w = torch.zeros(tgt.numel(), dtype=torch.float64)
    g_w[pos] = prod.sum(1)
    bound = torch.zeros_like(g_w)
    bound[pos] = (F + 8) * U * prod.abs().sum(1)
    return g_w, bound


# ---- the kernels' chains in fp32 numpy -------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64; the sum is rounded to float64 and then to
    float32 (a double rounding, which differs from the one rounding of fmaf in about one case in 2^29: of no weight in a
    check against half of a bound)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _chain(rows, wv, by, n_rows, F):
    """acc[by[p]] = fma(wv[p], rows[p], acc[by[p]]) over p in ascending order."""
    acc = np.zeros((n_rows, F), dtype=np.float32)
    for p in range(len(by)):
        acc[by[p]] = _fma(np.broadcast_to(wv[p], (F,)), rows[p], acc[by[p]])
    return acc


def emulate_fwd(x, w, tgt, src, valid, Nt):
    x = np.asarray(x, dtype=np.float32)
    pos = np.nonzero(np.asarray(valid))[0]
    i, j = np.asarray(tgt)[pos], np.asarray(src)[pos]
    wv = np.ones(len(pos), dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32).reshape(-1)[pos]
    return _chain(x[j], wv, i, Nt, x.shape[1]), np.bincount(i, minlength=Nt)


def emulate_bwd_x(g_out, w, tgt, src, valid, Ns):
    g = np.asarray(g_out, dtype=np.float32)
    pos = np.nonzero(np.asarray(valid))[0]
    i, j = np.asarray(tgt)[pos], np.asarray(src)[pos]
    wv = np.ones(len(pos), dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32).reshape(-1)[pos]
    return _chain(g[i], wv, j, Ns, g.shape[1])


def lanes_of(F):
    return 16 if F <= 64 else (32 if F <= 128 else 64)


def emulate_bwd_w(g_out, x, tgt, src, valid):
    """g_w [P] as the by-target kernel forms it: lane l adds the products of the features 4l .. 4l+3 in ascending order
    from 0, then the xor butterfly over the row's lanes."""
    g, x = np.asarray(g_out, dtype=np.float32), np.asarray(x, dtype=np.float32)
    F = x.shape[1]
    L = lanes_of(F)
    pos = np.nonzero(np.asarray(valid))[0]
    i, j = np.asarray(tgt)[pos], np.asarray(src)[pos]
    prod = np.zeros((len(pos), 4 * L), dtype=np.float32)
    prod[:, :F] = g[i] * x[j]                       # one rounding per product; features past F are not added at all
    prod = prod.reshape(len(pos), L, 4)
    s = np.zeros((len(pos), L), dtype=np.float32)
    for c in range(4):
        s = s + prod[:, :, c]                        # adding the 0 of a missing feature changes no bit of a partial sum
    off = L // 2
    while off >= 1:
        s = s + s[:, np.arange(L) ^ off]
        off //= 2
    out = np.zeros(len(np.asarray(tgt)), dtype=np.float32)
    out[pos] = s[:, 0]
    return out


class FakeNative:
    """Stand-ins for deepmetv2_amd._native._weighted_sum_fwd / _weighted_sum_bwd on CPU tensors over the emulation."""

    @staticmethod
    def _positions(idx, rowptr, Ns):
        return positions_of_table(idx, Ns) if rowptr is None else positions_of_list(idx, rowptr, Ns)

    def fwd(self, x, w, idx, rowptr, num_targets):
        pos = self._positions(idx, rowptr, x.shape[0])
        out, count = emulate_fwd(x.detach().numpy(), None if w is None else w.detach().numpy(), *pos, num_targets)
        return torch.from_numpy(out), torch.from_numpy(count).int()

    def bwd(self, g_out, x, w, idx, rowptr, tgt, rev_ptr, rev_pos, need_x=True, need_w=True):
        pos = self._positions(idx, rowptr, x.shape[0])
        wn = None if w is None else w.detach().numpy()
        g_x = torch.from_numpy(emulate_bwd_x(g_out.detach().numpy(), wn, *pos, x.shape[0])) if need_x else None
        g_w = torch.from_numpy(emulate_bwd_w(g_out.detach().numpy(), x.detach().numpy(), *pos)) if need_w else None
        return g_x, g_w

    def install(self, monkeypatch):
        import deepmetv2_amd._native as nat
        monkeypatch.setattr(nat, "_weighted_sum_fwd", self.fwd)
        monkeypatch.setattr(nat, "_weighted_sum_bwd", self.bwd)


# ---- the kernel cases of tests/test_gpu_weighted_sum.py (and of the emulation check in the host tests) ---------------------------
WIDTHS = (1, 3, 16, 17, 64)
FEATURES = (1, 3, 4, 5, 64, 65, 128, 129, 256)
KERNEL_CASES = list(dict.fromkeys(
    [("table", 5, k, None) for k in WIDTHS] + [("table", 64, k, None) for k in (16, 17)] +
    [("table", F, 3, None) for F in FEATURES] + [("list", F, 0, None) for F in FEATURES] + [("table", 12, 16, 57)]))

_cache = {}


def kernel_case(kind, F, k=3, num_src=None, seed=0):
    """(x [Ns, F], w [P], g_out [Nt, F], graph dict, (tgt, src, valid), Nt): the graphs of tests/pna_cases.py, normal draws
    for x, w and g_out; a tenth of the weights is exactly 0, about half of the rest negative."""
    import pna_cases as pc
    key = (kind, F, k, num_src, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(4000 + 131 * seed + F + 7 * k)
        if kind == "table":
            nbr, _event = pc.table_graph(k, 20 + k + seed, num_src=num_src)
            Ns = num_src or nbr.shape[0]
            graph, pos, Nt = {"nbr": nbr}, positions_of_table(nbr, Ns), nbr.shape[0]
        else:
            src, rowptr = pc.list_graph(31 + seed)
            Ns = Nt = rowptr.numel() - 1
            graph, pos = {"src": src, "rowptr": rowptr}, positions_of_list(src, rowptr, Ns)
        x = torch.randn(Ns, F, generator=g)
        w = torch.randn(pos[0].numel(), generator=g)
        w[torch.rand(w.numel(), generator=g) < 0.1] = 0.0
        g_out = torch.randn(Nt, F, generator=g)
        _cache[key] = (x, w, g_out, graph, pos, Nt)
    return _cache[key]


# ---- graphs for the layers ---------------------------------------------------------------------------------------------------
def keep_one_loop(tgt, src, valid):
    """valid with every written self loop but a node's first dropped: upstream keeps one loop per node, the package
    counts all of them (the stated deviation), so the layer tests run where the two agree."""
    valid = valid.clone()
    seen = set()
    for p in torch.nonzero(valid & (tgt == src)).view(-1).tolist():
        if int(tgt[p]) in seen:
            valid[p] = False
        seen.add(int(tgt[p]))
    return valid


def layer_graph(kind, seed=0):
    """{graph, pos, N, w}: the 201-node table (k = 16) or the 140-node list of tests/pna_cases.py with a few written self
    loops added and at most one kept per node; w [P]: positive weights per position (a GCN degree must not vanish by
    cancellation), drawn for every slot, empty ones included."""
    import pna_cases as pc
    key = ("layer", kind, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(5000 + seed)
        if kind == "table":
            nbr, _event = pc.table_graph(16, 60 + seed)
            nbr = nbr.clone()
            rows = torch.arange(10, 60, 5)
            nbr[rows, 1] = rows.to(nbr.dtype)                       # written loops, not in the first slot
            tgt, src, valid = positions_of_table(nbr, nbr.shape[0])
            keep = keep_one_loop(tgt, src, valid)
            nbr.view(-1)[valid & ~keep] = -1
            graph, N = {"nbr": nbr}, nbr.shape[0]
            pos = positions_of_table(nbr, N)
        else:
            src, rowptr = pc.list_graph(61 + seed)
            N = rowptr.numel() - 1
            tgt, src, valid = positions_of_list(src, rowptr, N)
            src = src.clone()
            at = torch.arange(0, src.numel(), 37)
            src[at] = tgt[at]                                        # written loops; the hub gets several
            keep = keep_one_loop(tgt, src, valid)
            tgt, src = tgt[keep], src[keep]
            rowptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(tgt, minlength=N).cumsum(0)])
            graph = {"src": src.to(torch.int32), "rowptr": rowptr.to(torch.int32)}
            pos = positions_of_list(graph["src"], graph["rowptr"], N)
        w = 0.1 + 1.5 * torch.rand(pos[0].numel(), generator=g)
        _cache[key] = {"graph": graph, "pos": pos, "N": N, "w": w}
    return _cache[key]


# ---- PyG's layers as published, per edge -------------------------------------------------------------------------------------
def _sum(msg, tgt, N):
    return torch.zeros((N, msg.shape[1]), dtype=msg.dtype).index_add(0, tgt, msg)


def _aggregate(x_src, src, tgt, w, N, how):
    msg = x_src.index_select(0, src)
    if w is not None:
        msg = msg * w.view(-1, 1)
    if how == "max":
        idx = tgt.view(-1, 1).expand_as(msg)
        return torch.zeros((N, msg.shape[1]), dtype=msg.dtype).scatter_reduce(0, idx, msg, "amax", include_self=False)
    out = _sum(msg, tgt, N)
    if how == "mean":
        out = out / torch.bincount(tgt, minlength=N).clamp(min=1).to(out.dtype).view(-1, 1)
    return out


def upstream_gcn_norm(src, tgt, w, N, improved=False, add_self_loops=True):
    """(src, tgt, normalised weight) as torch_geometric.nn.conv.gcn_conv.gcn_norm: add_remaining_self_loops with
    fill 2 (improved) or 1, deg by target, deg^-1/2 with inf -> 0."""
    if add_self_loops:
        loop = src == tgt
        loop_w = torch.full((N,), 2.0 if improved else 1.0, dtype=w.dtype).index_put((src[loop],), w[loop])
        ar = torch.arange(N)
        src, tgt, w = torch.cat([src[~loop], ar]), torch.cat([tgt[~loop], ar]), torch.cat([w[~loop], loop_w])
    deg = torch.zeros(N, dtype=w.dtype).index_add(0, tgt, w)
    zero = deg == 0
    dinv = torch.where(zero, torch.zeros_like(deg), torch.where(zero, torch.ones_like(deg), deg).pow(-0.5))
    return src, tgt, dinv[src] * w * dinv[tgt]


class UpstreamGCNConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, improved=False, add_self_loops=True, normalize=True, bias=True):
        super().__init__()
        self.improved, self.add_self_loops, self.normalize = improved, add_self_loops, normalize
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if bias else None

    def forward(self, x, src, tgt, w=None):
        N = x.shape[0]
        if self.normalize:
            w = torch.ones(src.numel(), dtype=x.dtype) if w is None else w
            src, tgt, w = upstream_gcn_norm(src, tgt, w, N, self.improved, self.add_self_loops)
        out = _aggregate(self.lin(x), src, tgt, w, N, "sum")
        return out if self.bias is None else out + self.bias


class UpstreamGraphConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, aggr="add", bias=True):
        super().__init__()
        in_src, in_dst = in_channels if isinstance(in_channels, tuple) else (in_channels, in_channels)
        self.aggr = aggr
        self.lin_rel = torch.nn.Linear(in_src, out_channels, bias=bias)
        self.lin_root = torch.nn.Linear(in_dst, out_channels, bias=False)

    def forward(self, x, src, tgt, w=None):
        x_src, x_dst = x if isinstance(x, tuple) else (x, x)
        out = _aggregate(x_src, src, tgt, w, x_dst.shape[0], "mean" if self.aggr == "mean" else "sum")
        return self.lin_rel(out) + self.lin_root(x_dst)


class UpstreamSAGEConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, aggr="mean", normalize=False, root_weight=True, project=False, bias=True):
        super().__init__()
        in_src, in_dst = in_channels if isinstance(in_channels, tuple) else (in_channels, in_channels)
        self.aggr, self.normalize, self.root_weight, self.project = aggr, normalize, root_weight, project
        if project:
            self.lin = torch.nn.Linear(in_src, in_src, bias=True)
        self.lin_l = torch.nn.Linear(in_src, out_channels, bias=bias)
        if root_weight:
            self.lin_r = torch.nn.Linear(in_dst, out_channels, bias=False)

    def forward(self, x, src, tgt, w=None):
        x_src, x_dst = x if isinstance(x, tuple) else (x, x)
        if self.project:
            x_src = self.lin(x_src).relu()
        out = self.lin_l(_aggregate(x_src, src, tgt, None, x_dst.shape[0], {"add": "sum"}.get(self.aggr, self.aggr)))
        if self.root_weight:
            out = out + self.lin_r(x_dst)
        return torch.nn.functional.normalize(out, p=2.0, dim=-1) if self.normalize else out


class UpstreamGINConv(torch.nn.Module):
    def __init__(self, nn, eps=0.0, train_eps=False):
        super().__init__()
        self.nn = nn
        if train_eps:
            self.eps = torch.nn.Parameter(torch.full((1,), float(eps)))
        else:
            self.register_buffer("eps", torch.full((1,), float(eps)))

    def forward(self, x, src, tgt, w=None):
        x_src, x_dst = x if isinstance(x, tuple) else (x, x)
        return self.nn(_aggregate(x_src, src, tgt, None, x_dst.shape[0], "sum") + (1 + self.eps) * x_dst)


# ---- the layer cases of the host and GPU tests -------------------------------------------------------------------------------
CIN, COUT = 12, 8
# name: (the package's class, its restatement, (in, out) channels, options, takes edge_weight)
LAYERS = {
    "gcn": ("GCNConv", UpstreamGCNConv, (CIN, COUT), {}, True),
    "gcn_unweighted": ("GCNConv", UpstreamGCNConv, (CIN, COUT), {}, False),
    "gcn_improved": ("GCNConv", UpstreamGCNConv, (CIN, COUT), {"improved": True}, True),
    "gcn_no_self_loops": ("GCNConv", UpstreamGCNConv, (CIN, COUT), {"add_self_loops": False}, True),
    "gcn_no_normalize": ("GCNConv", UpstreamGCNConv, (CIN, COUT), {"normalize": False}, True),
    "graph_add": ("GraphConv", UpstreamGraphConv, (CIN, COUT), {"aggr": "add"}, True),       # aggregates lin_rel's output
    "graph_mean": ("GraphConv", UpstreamGraphConv, (COUT, CIN), {"aggr": "mean"}, True),      # aggregates x
    "sage_mean": ("SAGEConv", UpstreamSAGEConv, (CIN, COUT), {"aggr": "mean"}, False),
    "sage_sum": ("SAGEConv", UpstreamSAGEConv, (CIN, COUT), {"aggr": "sum", "root_weight": False}, False),
    "sage_max": ("SAGEConv", UpstreamSAGEConv, (CIN, COUT), {"aggr": "max"}, False),
    "sage_normalize_project": ("SAGEConv", UpstreamSAGEConv, (CIN, COUT), {"normalize": True, "project": True}, False),
    "gin": ("GINConv", UpstreamGINConv, (CIN, COUT), {"eps": 0.3, "train_eps": True}, False),
}


def _mlp(cin, cout):
    return torch.nn.Sequential(torch.nn.Linear(cin, cout), torch.nn.ReLU(), torch.nn.Linear(cout, cout))


def build_layer(name, channels=None):
    """(the package's layer, its float64 restatement, its fp32 restatement) on the same random parameters; every 1-D
    parameter (the biases, GCN's zero-initialised one included) is drawn too."""
    import deepmetv2_amd as dm
    cls, up, (cin, cout), kwargs, _weighted = LAYERS[name]
    cin = channels if channels is not None else cin
    torch.manual_seed(7)
    make = (lambda c: c(_mlp(cin[0] if isinstance(cin, tuple) else cin, cout), **kwargs)) if cls == "GINConv" \
        else (lambda c: c(cin, cout, **kwargs))
    ours = make(getattr(dm, cls))
    with torch.no_grad():
        for p in ours.parameters():
            if p.dim() == 1 and p.numel() > 1:
                p.normal_(generator=torch.Generator().manual_seed(8))
    ref64, ref32 = make(up).double(), make(up)
    ref64.load_state_dict(ours.state_dict())
    ref32.load_state_dict(ours.state_dict())
    return ours, ref64, ref32


def layer_tensors(mod, x, graph_args, w, g, w_keep=None):
    """[(name, tensor)]: out, g_x (per x tensor), g_w (the entries w_keep selects) and every parameter's gradient of
    mod(x, *graph_args[, w]) under the upstream gradient g."""
    xs = tuple(t.clone().requires_grad_(True) for t in (x if isinstance(x, tuple) else (x,)))
    ww = None if w is None else w.clone().requires_grad_(True)
    for p in mod.parameters():
        p.grad = None
    out = mod(xs if len(xs) == 2 else xs[0], *graph_args, *(() if ww is None else (ww,)))
    out.backward(g.to(out.dtype).to(out.device))
    res = [("out", out.detach())] + [(f"g_x{n}", t.grad) for n, t in enumerate(xs)]
    if ww is not None:
        gw = ww.grad.reshape(-1)
        res.append(("g_w", gw if w_keep is None else gw[w_keep.to(gw.device)]))
    return res + [(n, p.grad) for n, p in mod.named_parameters()]

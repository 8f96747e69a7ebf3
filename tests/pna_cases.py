"""Inputs shared by tests/test_pna_host.py and tests/test_gpu_pna.py: small graphs with every edge case the kernels of
csrc/multi_aggr.hip meet, the data regimes, and the condition on the inputs (no reference variance near the 1e-5 clamp of
the standard deviation) made to hold by construction.  Everything is a CPU tensor; references are cached per case."""
import functools

import torch

import pna_reference as pr

SIZES = (90, 7, 104)        # three ragged events, 201 nodes
DATA = ("normal", "offset1000", "offset-50", "ints", "const_rows")


def make_x(N, F, data, g, event=None):
    if data == "normal":
        return torch.randn(N, F, generator=g)
    if data == "offset1000":
        return 1000.0 + torch.randn(N, F, generator=g)
    if data == "offset-50":
        return -50.0 + 0.01 * torch.randn(N, F, generator=g)
    if data == "ints":
        return torch.randint(-8, 9, (N, F), generator=g).float()
    if data == "const_rows":        # one small integer per event and feature: every row repeats one value
        per_event = torch.randint(-8, 9, (int(event.max()) + 1, F), generator=g).float()
        return per_event[event]
    raise ValueError(data)


def _event_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def table_graph(k, seed, dense=False, sizes=SIZES, num_src=None):
    """nbr[N, k] int32 over three ragged events: random neighbours of the node's own event with duplicates; unless
    `dense`, blanked -1 slots anywhere, one id past the sources, fully empty rows and rows with one valid slot.  `dense`
    keeps every row at k, 1 or 0 valid slots (for the data regimes that need long rows, see clear_the_clamp)."""
    g = torch.Generator().manual_seed(seed)
    event = _event_of(sizes)
    N = event.numel()
    lo = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(sizes).cumsum(0)])[:-1][event]
    size = torch.tensor(sizes)[event]
    nbr = (lo.view(-1, 1) + (torch.rand(N, k, generator=g) * size.view(-1, 1)).long().clamp(max=size.view(-1, 1) - 1))
    if num_src is not None:      # a bipartite table: ids into another set
        nbr = (torch.rand(N, k, generator=g) * num_src).long().clamp(max=num_src - 1)
    if not dense:
        nbr[torch.rand(N, k, generator=g) < 0.2] = -1
        nbr[5, k // 2] = (num_src or N) + 3          # an id outside [0, Ns): skipped
    nbr[torch.arange(3, N, 17)] = -1                  # fully empty rows
    one = torch.arange(8, N, 23)                      # rows with one valid slot, not the first
    keep = nbr[one, 0].clamp(min=0)
    nbr[one] = -1
    nbr[one, k - 1] = keep
    return nbr.to(torch.int32), event


def list_graph(seed, N=140, hub=300, short=True):
    """(src[E], rowptr[N+1]) int32, grouped by target: in-degrees 0, 1, 63, 64, 65, one hub of `hub` and (short) 2 and a
    few random ones; sources N-10.. have no outgoing edge."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.zeros(N, dtype=torch.long)
    deg[1], deg[4], deg[5], deg[6], deg[9] = 1, 63, 64, 65, hub
    deg[20:30] = 1
    if short:
        deg[2] = 2
        deg[40:80] = torch.randint(0, 6, (40,), generator=g)
    E = int(deg.sum())
    src = torch.randint(0, N - 10, (E,), generator=g)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
    return src.to(torch.int32), rowptr.to(torch.int32)


def _fast_var(x, tgt, src, valid, Nt):
    pos = torch.nonzero(valid).view(-1)
    i, j = tgt[pos], src[pos]
    x = x.double()
    n = torch.bincount(i, minlength=Nt).double().clamp(min=1).view(-1, 1)
    mean = torch.zeros(Nt, x.shape[1], dtype=torch.float64).index_add_(0, i, x[j]) / n
    return torch.zeros_like(mean).index_add_(0, i, (x[j] - mean[i]) ** 2) / n


def clear_the_clamp(x, tgt, src, valid, Nt):
    """x with the condition on the inputs made to hold: where a row's float64 variance is neither 0 nor outside
    [2.5e-6, 4e-5] (two or three nearly equal draws), the feature of the row's first source is moved by 1 to 2.5.  Which
    elements move depends on the float64 reference alone."""
    x = x.clone()
    pos = torch.nonzero(valid).view(-1)
    first = torch.full((Nt,), -1, dtype=torch.long)
    first.scatter_reduce_(0, tgt[pos], pos, "amin", include_self=False)
    for _ in range(50):
        var = _fast_var(x, tgt, src, valid, Nt)
        bad = (var != 0) & (var >= 2.0e-6) & (var <= 5e-5)
        if not bool(bad.any()):
            return x
        i, f = torch.nonzero(bad, as_tuple=True)
        x[src[first[i]], f] += 1.0 + 0.25 * (i % 7).float()      # by the row: two rows that share both sources part too
    raise AssertionError("the inputs could not be moved away from the clamp")


@functools.lru_cache(maxsize=None)
def case(kind, F, data, seed, k=3, num_src=None):
    """(x [Ns, F], graph dict, (tgt, src, valid), Nt, reference stats) of a named case; kind 'table' or 'list'.
    The cancellation regimes need rows of 0, 1 or many entries (a variance of a few draws of 0.01 N(0,1) falls into the
    clamp's neighbourhood in most rows): their graphs are the dense / long-row ones."""
    assert data in DATA, data
    g = torch.Generator().manual_seed(1000 + seed)
    long_rows = data in ("offset1000", "offset-50")
    if kind == "table":
        nbr, event = table_graph(k, seed, dense=long_rows, num_src=num_src)
        Ns = num_src or nbr.shape[0]
        x = make_x(Ns, F, data, g, event if num_src is None else torch.zeros(Ns, dtype=torch.long))
        graph = {"nbr": nbr}
        pos = pr.positions_of_table(nbr, Ns)
        Nt = nbr.shape[0]
    else:
        src, rowptr = list_graph(seed, short=not long_rows)
        Ns = Nt = rowptr.numel() - 1
        x = make_x(Ns, F, data, g, torch.zeros(Ns, dtype=torch.long))
        graph = {"src": src, "rowptr": rowptr}
        pos = pr.positions_of_list(src, rowptr, Ns)
    if data not in ("ints", "const_rows"):
        x = clear_the_clamp(x, *pos, Nt)
    ref = pr.stats(x, *pos, Nt)
    assert pr.clamp_is_clear(ref), (kind, F, data, seed)
    return x, graph, pos, Nt, ref


def upstream_gradient(aggrs, Nt, F, groups, seed):
    """g_out [Nt, G, A, F/G] fp32 for a case's backward."""
    g = torch.Generator().manual_seed(77 + seed)
    return torch.randn(Nt, groups, len(aggrs), F // groups, generator=g)

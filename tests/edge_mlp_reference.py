"""Float64 references and the bf16 recipe emulation of the two-layer edge MLP (Linear - ELU - Linear [- ELU]
[- BatchNorm1d]) over an explicit edge index, shared by the GPU tests of the edge-MLP routes.  Test infrastructure only:
plain functions, no fixtures."""
import copy

import torch


def ends(ei, flow):
    return (ei[1], ei[0]) if flow == "source_to_target" else (ei[0], ei[1])     # (target, source), rule R5


def emulate(nn, x, ei, aggr, flow):
    """The kernel's recipe in torch: (out, post-BatchNorm messages [E, H2]).  P and Q are formed in float64 and kept as
    fp32, h1 = ELU(P_tgt + Q_src) in fp32, z2 from bf16(h1) and bf16(W2) (exact products, float64 sums, kept as fp32)."""
    bf = lambda t: t.to(torch.bfloat16).to(torch.float64)
    mods = list(copy.deepcopy(nn).to(x.device))
    bn = mods.pop() if isinstance(mods[-1], torch.nn.BatchNorm1d) else None
    l1, l2, act2 = mods[0], mods[2], len(mods) == 4
    tgt, src = ends(ei, flow)
    N, Hin = x.shape
    with torch.no_grad():
        W1 = l1.weight.double()
        b1 = l1.bias.double() if l1.bias is not None else 0.0
        xd = x.double()
        P = (xd @ (W1[:, :Hin] - W1[:, Hin:]).T + b1).float()
        Q = (xd @ W1[:, Hin:].T).float()
        h1 = torch.nn.functional.elu(P[tgt] + Q[src])
        z = (bf(h1) @ bf(l2.weight).T).float()
        if l2.bias is not None:
            z = z + l2.bias
        m = torch.nn.functional.elu(z) if act2 else z
        if bn is not None:
            if bn.training:
                mean, var = m.double().mean(0), m.double().var(0, unbiased=False)
            else:
                mean, var = bn.running_mean.double(), bn.running_var.double()
            a = bn.weight.double() / torch.sqrt(var + bn.eps)
            m = (a * m.double() + (bn.bias.double() - mean * a)).float()
        H2 = m.shape[1]
        idx = tgt.view(-1, 1).expand(-1, H2)
        if aggr == "max":
            out = torch.zeros((N, H2), dtype=m.dtype, device=m.device).scatter_reduce(0, idx, m, "amax", include_self=False)
        else:
            out = torch.zeros((N, H2), dtype=m.dtype, device=m.device).index_add_(0, tgt, m)
            if aggr == "mean":
                out = out / torch.bincount(tgt, minlength=N).clamp(min=1).to(m.dtype).view(-1, 1)
    return out, m


def kernel_winners(nn, x, ei, flow, route="bf16"):
    """(grouped edge index [2, E], winners [N, H2]): the winning grouped edge position of each target's maximum after
    the norm, as the forward state of the route's kernel records it (-1: no in-edge).  The float64 composition takes these."""
    from deepmetv2_amd import _native
    from deepmetv2_amd.conv import _as_mlp2
    from deepmetv2_amd.graph import edge_list_from_edge_index
    l1, l2, act2, bn = _as_mlp2(copy.deepcopy(nn).to(x.device))
    edges = edge_list_from_edge_index(ei, x.shape[0], flow)
    mode = 0 if bn is None else (1 if bn.training else 2)
    _out, (_pq, _agg, win, bnstat) = getattr(_native, f"edge_mlp_fwd_{route}")(
        x, edges.rowptr, edges.src, edges.tgt, l1.weight, l1.bias, l2.weight, l2.bias, act2, "max", mode,
        bn.weight if bn is not None else None, bn.bias if bn is not None else None, 1e-5, 0.1,
        bn.running_mean if mode == 2 else None, bn.running_var if mode == 2 else None, None)
    w = win[0].long()
    if mode:
        w = torch.where(bnstat[0] < 0, win[1].long(), w)        # a < 0: the minimum before the norm wins
    deg = (edges.rowptr[1:] - edges.rowptr[:-1]).view(-1, 1)
    grouped = torch.stack([edges.src.long(), edges.tgt.long()])    # source -> target, grouped by target
    return grouped, torch.where(deg > 0, w, torch.full_like(w, -1))


def ref64(nn, x, ei, aggr, flow, g, win=None):
    """float64 composition of the same layer (generic form: edge features, nn, aggregation): (out, gx, grads)"""
    nn64 = copy.deepcopy(nn).double().to(x.device)
    tgt, src = ends(ei, flow)
    N = x.shape[0]
    xx = x.detach().double().requires_grad_(True)
    m = nn64(torch.cat([xx[tgt], xx[src] - xx[tgt]], dim=1))
    if aggr == "max":
        out = torch.where(win >= 0, m.gather(0, win.clamp(min=0)), torch.zeros((), dtype=m.dtype, device=m.device))
    else:
        out = torch.zeros((N, m.shape[1]), dtype=m.dtype, device=m.device).index_add(0, tgt, m)
        if aggr == "mean":
            out = out / torch.bincount(tgt, minlength=N).clamp(min=1).to(m.dtype).view(-1, 1)
    out.backward(g.double())
    grads = {n: p.grad.detach() for n, p in nn64.named_parameters() if p.grad is not None}
    return out.detach(), xx.grad.detach(), grads


def max64(nn, x, ei, flow):
    """float64 maximum per target of the same layer's messages, by scatter amax: no winners taken from any kernel"""
    nn64 = copy.deepcopy(nn).double().to(x.device)
    tgt, src = ends(ei, flow)
    with torch.no_grad():
        xx = x.detach().double()
        m = nn64(torch.cat([xx[tgt], xx[src] - xx[tgt]], dim=1))
        idx = tgt.view(-1, 1).expand(-1, m.shape[1])
        return torch.zeros((x.shape[0], m.shape[1]), dtype=m.dtype, device=m.device).scatter_reduce(0, idx, m, "amax",
                                                                                                     include_self=False)

"""float64 restatement of torch_geometric.nn.GravNetConv over a given neighbour table, on the CPU.

PyG's forward is
    h = lin_h(x_l); s_l = lin_s(x_l); s_r = lin_s(x_r)
    edge_weight = exp(-10 * (s_l[src] - s_r[tgt]).pow(2).sum(-1))
    out = propagate(message = h[src] * edge_weight, aggr = ['mean', 'max'])        # [N_r, 2P]
    return lin_out1(x_r) + lin_out2(out)
Here the edges are the valid slots of a fixed-width table nbr[Nt, k] (-1 = empty): slot t of row i is the edge
nbr[i, t] -> i.  Empty slots are skipped, the max breaks ties to the lowest slot, a row without a valid slot gives zeros.
The max is taken over the messages that are numbers (nonfinite_contract.nan_skipping_max: a NaN never wins and never
blocks); a channel of a non-empty row whose messages are all NaN is NaN with no winner.
"""
import torch


def messages(h, s_src, s_tgt, nbr):
    """(msg[Nt, k, P] with zeros in empty slots, valid[Nt, k]).  Only valid slots enter the arithmetic, so a non-finite
    coordinate of a node that is nobody's neighbour and has an empty row touches nothing."""
    nbr = nbr.long()
    Nt, k = nbr.shape
    valid = nbr >= 0
    i, t = valid.nonzero(as_tuple=True)
    j = nbr[i, t]
    d = (s_src[j] - s_tgt[i]).pow(2).sum(-1)
    m = torch.exp(-10.0 * d).unsqueeze(-1) * h[j]
    msg = torch.zeros((Nt, k, h.shape[1]), dtype=h.dtype).index_put((i, t), m)
    return msg, valid


def lowest_slot_argmax(msg, valid):
    """arg[Nt, P] int64: the lowest valid slot holding the row's maximum over the messages that are numbers; k (one past
    the last slot) for an empty row and for a channel whose messages are all NaN."""
    from nonfinite_contract import nan_skipping_max
    k = msg.shape[1]
    _top, pos = nan_skipping_max(msg.detach().transpose(1, 2), valid.unsqueeze(1).expand(-1, msg.shape[2], -1))
    return torch.where(pos < 0, torch.full_like(pos, k), pos)


def aggregate(h, s, nbr, s_dst=None, arg=None):
    """(out[Nt, 2P] = [mean | max], bar[Nt] = sum over valid t of |h_j|_inf, msg, valid, arg).  One set: s_dst None.
    arg (int64 [Nt, P], optional): route the max, and so its backward, through these slots instead of the reference's own
    lowest-slot winners; entries of empty rows are ignored."""
    s_tgt = s if s_dst is None else s_dst
    msg, valid = messages(h, s, s_tgt, nbr)
    cnt = valid.sum(1)
    has = (cnt > 0).unsqueeze(-1)
    mean = msg.sum(1) / cnt.clamp(min=1).unsqueeze(-1).to(msg.dtype)
    own = lowest_slot_argmax(msg, valid)
    use = own if arg is None else arg.long()
    none = has & (use >= msg.shape[1])                      # entries, but no number among a channel's messages
    use = torch.where(has, use, torch.zeros_like(use)).clamp(max=msg.shape[1] - 1)
    mx = torch.where(has, msg.gather(1, use.unsqueeze(1)).squeeze(1), torch.zeros_like(mean))
    mx = torch.where(none, torch.full_like(mx, float("nan")), mx)
    with torch.no_grad():
        hinf = h.abs().amax(1) if h.shape[0] else h.new_zeros(1)      # no source: every slot is empty
        bar = torch.where(valid, hinf[nbr.long().clamp(min=0)], torch.zeros((), dtype=h.dtype)).sum(1)
    return torch.cat([mean, mx], 1), bar, msg, valid, own


class RefGravNetConv(torch.nn.Module):
    """The four Linears of GravNetConv in float64, applied over a given table (the graph is an input here: the kNN
    search is tested on its own)."""

    def __init__(self, in_channels, out_channels, space_dimensions, propagate_dimensions):
        super().__init__()
        self.lin_s = torch.nn.Linear(in_channels, space_dimensions).double()
        self.lin_h = torch.nn.Linear(in_channels, propagate_dimensions).double()
        self.lin_out1 = torch.nn.Linear(in_channels, out_channels, bias=False).double()
        self.lin_out2 = torch.nn.Linear(2 * propagate_dimensions, out_channels).double()

    def forward(self, x, nbr, x_dst=None, arg=None):
        s, h = self.lin_s(x), self.lin_h(x)
        s_dst = None if x_dst is None else self.lin_s(x_dst)
        self.coords = [t for t in (s, s_dst) if t is not None and t.requires_grad]      # their .grad: the terms lin_s.bias's gradient sums
        for t in self.coords:
            t.retain_grad()
        agg = aggregate(h, s, nbr, s_dst, arg)[0]
        return self.lin_out1(x if x_dst is None else x_dst) + self.lin_out2(agg)

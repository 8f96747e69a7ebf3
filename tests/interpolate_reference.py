"""float64 restatement of torch_geometric.nn.unpool.knn_interpolate over a given neighbour table, on the CPU.

PyG's forward, after y_idx, x_idx = knn(pos_x, pos_y, k, batch_x, batch_y), is
    diff = pos_x[x_idx] - pos_y[y_idx]; squared_distance = (diff * diff).sum(-1, keepdim=True)
    weights = 1.0 / torch.clamp(squared_distance, min=1e-16)                                  (under no_grad)
    y = scatter(x[x_idx] * weights, y_idx, 0, pos_y.size(0), 'sum') / scatter(weights, y_idx, 0, pos_y.size(0), 'sum')
Here the edges are the valid slots of a fixed-width table nbr[Nt, k] (-1, or any id outside [0, Ns), = empty): slot t of
row i is the edge nbr[i, t] -> i, and the squared distances are given (dist[Nt, k] fp32, the table's own; the value in an
empty slot is ignored).  The weights are normalised before the sum, r_t = w_t / W_i, as include/dmet.h states it; the
clamp is at the fp32 value of 1e-16, which is what upstream's clamp of an fp32 tensor compares with too.
"""
import torch

MIN_D = float(torch.tensor(1e-16, dtype=torch.float32))


def weights(nbr, dist32, num_sources):
    """(r[Nt, k] float64 with zeros in empty slots, W[Nt] float64, valid[Nt, k], j[Nt, k] int64 with 0 in empty slots).
    Validity is told by the id alone."""
    nbr = nbr.long()
    valid = (nbr >= 0) & (nbr < num_sources)
    w = torch.where(valid, 1.0 / dist32.double().clamp(min=MIN_D), torch.zeros((), dtype=torch.float64))
    W = w.sum(1)
    r = w / torch.where(W > 0, W, torch.ones_like(W)).unsqueeze(-1)
    return r, W, valid, torch.where(valid, nbr, torch.zeros_like(nbr))


def interpolate(x64, nbr, dist32):
    """(out[Nt, F], bar[Nt, F] = sum_t r_t |x[j_t, f]|, wsum[Nt] = W_i, valid[Nt, k]); out is differentiable in x64.  A
    row without a valid slot gives zeros and wsum 0."""
    Ns, F = x64.shape
    r, W, valid, j = weights(nbr, dist32, Ns)
    if Ns == 0:     # every slot is empty
        z = x64.new_zeros((nbr.shape[0], F))
        return z + x64.sum() * 0, z.clone(), W, valid
    rows = x64[j] * valid.unsqueeze(-1)                     # [Nt, k, F]
    out = (r.unsqueeze(-1) * rows).sum(1)
    with torch.no_grad():
        bar = (r.unsqueeze(-1) * rows.abs()).sum(1)
    return out, bar, W, valid


def source_side(g64, nbr, dist32, num_sources):
    """(g_x[Ns, F] = sum over the positions p = (i, t) holding j of r_p g[i], bar_g[Ns, F] = the same sum of r_p |g[i]|,
    n[Ns] = the length of source j's list): the backward of `interpolate`, written out."""
    r, _W, valid, j = weights(nbr, dist32, num_sources)
    Nt, k = nbr.shape
    F = g64.shape[1]
    i_idx, t_idx = valid.nonzero(as_tuple=True)
    src = j[i_idx, t_idx]
    rp = r[i_idx, t_idx].unsqueeze(-1)
    g_x = torch.zeros((num_sources, F), dtype=torch.float64).index_add_(0, src, rp * g64[i_idx])
    bar_g = torch.zeros((num_sources, F), dtype=torch.float64).index_add_(0, src, rp * g64[i_idx].abs())
    n = torch.bincount(src, minlength=num_sources)[:num_sources] if num_sources else torch.zeros(0, dtype=torch.int64)
    return g_x, bar_g, n

"""References of the segment reductions of csrc/segment.hip (mean, min, softmax, log_softmax, logsumexp) in float64, and
CPU stand-ins for the `_native._segment_*` entries so that scatter.py's index handling runs without a GPU.

The references take rows [E,H] grouped by a rowptr of n + 1 entries (well-formed: 0 = rowptr[0] <= ... <= rowptr[n] = E)
and are plain vectorised torch: a row maximum by scatter_reduce, sums by index_add_.  They are differentiable, so float64
autograd through them is the backward reference."""
import torch

U = 2.0 ** -24          # unit roundoff of fp32


def row_ids(rowptr):
    rp = rowptr.long().cpu()
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp.diff())


def lengths_rowptr(lengths):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths, dtype=torch.int64).cumsum(0)]).int()


def _row_max(s, ids, n):
    H = s.shape[1]
    return torch.full((n, H), -float("inf"), dtype=s.dtype).scatter_reduce(0, ids.view(-1, 1).expand(-1, H), s.detach(),
                                                                          "amax", include_self=True)


def mean_ref(src, rowptr):
    """float64 [n,H]: sum / max(count, 1)."""
    s = src.double()
    ids, n = row_ids(rowptr), rowptr.numel() - 1
    cnt = rowptr.long().cpu().diff().clamp(min=1).double().view(-1, 1)
    return torch.zeros((n, s.shape[1]), dtype=torch.float64).index_add(0, ids, s) / cnt


def min_ref(src, rowptr):
    """(out, arg) like _max_ref of tests/test_gpu_scatter.py, mirrored: per (row, channel) the lowest position among the
    entries equal to the minimum; out carries that entry's bits; an empty row gives 0 and arg = E."""
    E, H = src.shape
    ids, n = row_ids(rowptr), rowptr.numel() - 1
    idx = ids.view(-1, 1).expand(E, H)
    mn = torch.zeros(n, H, dtype=src.dtype).scatter_reduce(0, idx, src, "amin", include_self=False)
    eq = src == mn[ids]
    pos = torch.where(eq, torch.arange(E).view(-1, 1).expand(E, H), torch.full((E, H), E))
    arg = torch.full((n, H), E).scatter_reduce(0, idx, pos, "amin", include_self=True)
    out = torch.where(arg < E, src[arg.clamp(max=max(E - 1, 0)), torch.arange(H).view(1, -1)] if E else torch.zeros(n, H),
                      torch.zeros(n, H, dtype=src.dtype))
    return out, arg


def softmax_parts(src, rowptr):
    """(s - m, l, m, ids) in float64 with m the row maximum; differentiable in src."""
    s = src.double() if src.dtype != torch.float64 else src
    ids, n = row_ids(rowptr), rowptr.numel() - 1
    m = _row_max(s, ids, n)
    d = s - m[ids]
    l = torch.zeros((n, s.shape[1]), dtype=torch.float64).index_add(0, ids, d.exp())
    return d, l, m, ids


def softmax_ref(src, rowptr):
    d, l, _m, ids = softmax_parts(src, rowptr)
    return d.exp() / l[ids]


def log_softmax_ref(src, rowptr):
    d, l, _m, ids = softmax_parts(src, rowptr)
    return d - l.log()[ids]


def logsumexp_ref(src, rowptr):
    """m + log(l); 0 for an empty row."""
    _d, l, m, _ids = softmax_parts(src, rowptr)
    empty = (rowptr.long().cpu().diff() == 0).view(-1, 1)
    safe_m = torch.where(empty, torch.zeros_like(m), m)
    return torch.where(empty, torch.zeros_like(l), safe_m + torch.where(empty, torch.ones_like(l), l).log())


# ---- the backward bounds of tests/test_gpu_segment_reduce.py, per entry of grouped rows ---------------------------------
def _row_sum_of(t, rowptr):
    ids = row_ids(rowptr)
    return torch.zeros((rowptr.numel() - 1, t.shape[1]), dtype=t.dtype).index_add(0, ids, t)[ids]


def softmax_bwd_bound(src, g, rowptr, n_of):
    """test_softmax_backward: 4 (n + |s| + 8) u y (|g| + sum_row |y g|)."""
    src, g = src.double(), g.double()
    y = softmax_ref(src, rowptr)
    return 4 * (n_of + src.abs() + 8) * U * y * (g.abs() + _row_sum_of((y * g).abs(), rowptr))


def log_softmax_bwd_bound(src, g, rowptr, n_of, ref):
    """test_log_softmax_backward: 2 u (|ref| + p (3 n + 4 |y| + 19) sum_row |g|), p = exp(y)."""
    y = log_softmax_ref(src.double(), rowptr)
    return 2 * U * (ref.abs() + y.exp() * (3 * n_of + 4 * y.abs() + 19) * _row_sum_of(g.double().abs(), rowptr))


def logsumexp_bwd_bound(src, rowptr, n_of, ref):
    """test_logsumexp_backward: 2 (2 n + 4 |out| + |s - out| + 19) u |ref|."""
    src = src.double()
    out_of = logsumexp_ref(src, rowptr)[row_ids(rowptr)]
    return 2 * (2 * n_of + 4 * out_of.abs() + (src - out_of).abs() + 19) * U * ref.abs()


# ---- CPU stand-ins of the _native entries (fp32 in and out, float64 inside) ---------------------------------------------
def _segment_mean(src, rowptr, max_len=0):
    return mean_ref(src.detach(), rowptr).float()


def _segment_mean_bwd(g_out, rowptr, E, max_len=0):
    cnt = rowptr.long().diff().clamp(min=1).float().view(-1, 1)
    return (g_out / cnt)[row_ids(rowptr)].contiguous()


def _segment_min(src, rowptr, max_len=0):
    out, arg = min_ref(src.detach(), rowptr)
    E = src.shape[0]
    return out, torch.where(arg >= E, torch.full_like(arg, -1), arg).int()


def _segment_softmax_fwd(src, rowptr, log=False, max_len=0):
    s = src.detach()
    y = (log_softmax_ref if log else softmax_ref)(s, rowptr).float()
    return y, logsumexp_ref(s, rowptr).float()


def _segment_softmax_bwd(y, g, rowptr, log=False, max_len=0):
    ids, n = row_ids(rowptr), rowptr.numel() - 1
    yd, gd = y.double(), g.double()
    zero = torch.zeros((n, y.shape[1]), dtype=torch.float64)
    if log:
        return (gd - yd.exp() * zero.index_add(0, ids, gd)[ids]).float()
    return (yd * (gd - zero.index_add(0, ids, yd * gd)[ids])).float()


def _segment_logsumexp(src, rowptr, max_len=0):
    return logsumexp_ref(src.detach(), rowptr).float()


def _segment_logsumexp_bwd(src, out, g_out, rowptr, max_len=0):
    ids = row_ids(rowptr)
    return (g_out.double()[ids] * (src.double() - out.double()[ids]).exp()).float()


NAMES = ["_segment_mean", "_segment_mean_bwd", "_segment_min", "_segment_softmax_fwd", "_segment_softmax_bwd",
         "_segment_logsumexp", "_segment_logsumexp_bwd"]


def install(monkeypatch):
    """Replace the new `_native` entries by the stand-ins for the duration of a test (beside fake_native.install)."""
    import deepmetv2_amd._native as nat
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(nat, n, g[n])

"""Float64 restatements for csrc/event_norm.hip and deepmetv2_amd/event_norm.py: the upstream formulas of GraphNorm,
InstanceNorm, LayerNorm, PairNorm, GraphSizeNorm and MeanSubtractionNorm as torch_geometric publishes them (composed from
index_add / index_select over the batch vector, in whatever dtype they are given: float64 is the reference, float32 on the
CPU sets the layers' tolerance), the closed-form gradients of event_moments and of the three modes of event_normalize, an
fp32 numpy emulation of the three kernels' chains, the bounds the GPU tests hold the kernels to, and FakeKernels, which
stands in for the kernels where the host logic is tested without a GPU.

Notation: u = 2^-24, n the event's length, gamma_n = n u / (1 - n u).  Bounds against float64 on the same fp32 inputs:
  mean   gamma_n mean|x|
  var    (2n + 8) u var + ((n + 2) u mean|x|)^2        the two-walk form in any summation order (multi_aggr's bound)
  s1     gamma_n sum|g|
  s2     (gamma_n + 3u) sum|g xh|                        three roundings per term: x - shift, * scale, g *
  affine the same bits as the fp32 restatement: every operation is rounded once, in a fixed order
"""
import numpy as np
import torch

U = 2.0 ** -24
KERNEL_LONG = 1024                # the max_len hint from which the 1024-thread form runs
HINTS = (0, KERNEL_LONG)          # one hint per form

# the issue's lengths, then T-1, T, T+1 for every length at which a team of either form takes one more stride of rows:
# 8 rows per entry lane and stride, S = threads / CL entry lanes: 32 / 128 / 512 rows (wavefront form, CL = 16 / 4 / 1)
# and 512 / 2048 / 8192 rows (workgroup form); 1023..1025 is also the hint's own threshold
LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 0, 1023, 1024, 1025, 4500, 0,
           31, 32, 33, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193]
WIDTHS = (1, 2, 3, 4, 5, 16, 17, 32, 33, 64, 65, 100)
LAYER_WIDTHS = (3, 16, 64, 100)
LAYER_LENGTHS = LENGTHS[:18]      # "the ragged batch" of the issue


def rowptr_of(lengths):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(lengths, dtype=torch.long).cumsum(0)]).to(torch.int32)


def batch_of(lengths):
    return torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1 - n * U)


_cache = {}


def data(F, kind="gauss", lengths=None, seed=0):
    """x [N, F] fp32 for the ragged batch: 'gauss' N(0,1), 'offset' 1000 + N(0,1), 'int' integers in [-8, 8]."""
    lengths = LENGTHS if lengths is None else lengths
    key = (F, kind, tuple(lengths), seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(100 + 7 * F + seed)
        N = sum(lengths)
        if kind == "int":
            x = torch.randint(-8, 9, (N, F), generator=g).float()
        else:
            x = torch.randn(N, F, generator=g) + (1000.0 if kind == "offset" else 0.0)
        _cache[key] = x
    return _cache[key]


# ---- float64 statistics and their bounds -------------------------------------------------------------------------------------
def _spans(rowptr, N):
    rp = [min(max(int(v), 0), N) for v in rowptr.tolist()]
    return [(rp[b], max(rp[b + 1], rp[b])) for b in range(len(rp) - 1)]


def moments(x, rowptr):
    """(mean, var, bound_mean, bound_var) [B, F] in float64."""
    x = x.double()
    B, F = rowptr.numel() - 1, x.shape[1]
    mean, var, absm, n = (torch.zeros(B, F, dtype=torch.float64) for _ in range(4))
    for b, (lo, hi) in enumerate(_spans(rowptr, x.shape[0])):
        if hi > lo:
            mean[b] = x[lo:hi].mean(0)
            var[b] = ((x[lo:hi] - mean[b]) ** 2).mean(0)
            absm[b] = x[lo:hi].abs().mean(0)
            n[b] = hi - lo
    return mean, var, gamma(n) * absm, (2 * n + 8) * U * var + ((n + 2) * U * absm) ** 2


def dots(g, x, rowptr, shift, scale):
    """(s1, s2, bound_s1, bound_s2) in float64 on the fp32 operands."""
    g, x, shift, scale = g.double(), x.double(), shift.double(), scale.double()
    B, F = shift.shape
    s1, s2, b1, b2 = (torch.zeros(B, F, dtype=torch.float64) for _ in range(4))
    for b, (lo, hi) in enumerate(_spans(rowptr, x.shape[0])):
        term = g[lo:hi] * ((x[lo:hi] - shift[b]) * scale[b])
        s1[b], s2[b] = g[lo:hi].sum(0), term.sum(0)
        b1[b] = gamma(hi - lo) * g[lo:hi].abs().sum(0)
        b2[b] = (gamma(hi - lo) + 3 * U) * term.abs().sum(0)
    return s1, s2, b1, b2


def affine(x, rowptr, shift, k1, k0, g=None, ka=None):
    """The elementwise pass in x's own dtype with torch operators, one rounding per operation; zeros outside the events."""
    out = torch.zeros_like(x)
    for b, (lo, hi) in enumerate(_spans(rowptr, x.shape[0])):
        o = (x[lo:hi] - shift[b]) * k1[b] + k0[b]
        out[lo:hi] = o if g is None else g[lo:hi] * ka[b] + o
    return out


# ---- event_normalize in any dtype, forward from the definition, and the closed-form gradients ---------------------------------
def _stats(x, rowptr):
    B, F = rowptr.numel() - 1, x.shape[1]
    rows = []
    for lo, hi in _spans(rowptr, x.shape[0]):
        if hi > lo:
            m = x[lo:hi].mean(0)
            rows.append((m, ((x[lo:hi] - m) ** 2).mean(0)))
        else:
            rows.append((x.new_zeros(F), x.new_zeros(F)))
    return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


def _a_and_r(mean, var, alpha, eps, mode):
    if mode == "channel":
        A, q = alpha * mean, var + ((1 - alpha) * mean) ** 2
    elif mode == "graph":
        m = mean.mean(1, keepdim=True)
        A, q = m.expand_as(mean), (var + (mean - m) ** 2).mean(1, keepdim=True).expand_as(mean)
    else:
        A, q = mean, var.sum(1, keepdim=True).expand_as(mean)
    return A, 1 / torch.sqrt(q + eps)


def normalize(x, rowptr, alpha, weight, bias, eps, mode):
    """y from the definition (differentiable by autograd in every operand); alpha / weight / bias: [F] tensors."""
    mean, var = _stats(x, rowptr)
    A, r = _a_and_r(mean, var, alpha, eps, mode)
    return affine(x, rowptr, A, r * weight, bias.expand_as(A))


def normalize_grads(x, g, rowptr, alpha, weight, bias, eps, mode):
    """(g_x, g_alpha, g_weight, g_bias) in closed form: what the package's backward computes, in the operands' dtype."""
    mean, var = _stats(x, rowptr)
    A, r = _a_and_r(mean, var, alpha, eps, mode)
    B, F = mean.shape
    n = torch.tensor([max(hi - lo, 1) for lo, hi in _spans(rowptr, x.shape[0])], dtype=x.dtype).view(-1, 1)
    S1, S2 = torch.zeros_like(mean), torch.zeros_like(mean)
    for b, (lo, hi) in enumerate(_spans(rowptr, x.shape[0])):
        S1[b], S2[b] = g[lo:hi].sum(0), (g[lo:hi] * ((x[lo:hi] - A[b]) * r[b])).sum(0)
    ka = r * weight
    g_alpha = torch.zeros_like(alpha)
    if mode == "channel":
        G = ka * S1 - r * r * weight * S2 * (1 - alpha) * mean
        K1, K0 = -r * r * weight * S2 / n, -alpha * G / n
        g_alpha = -(mean * G).sum(0)
    elif mode == "graph":
        T1, T2 = (weight * S1).sum(1, keepdim=True), (weight * S2).sum(1, keepdim=True)
        K1, K0 = (-r * r * T2 / (F * n)).expand_as(mean), (-r * T1 / (F * n)).expand_as(mean)
    else:
        T2 = (weight * S2).sum(1, keepdim=True)
        K1, K0 = (-r * r * T2 / n).expand_as(mean), -ka * S1 / n
    return affine(x, rowptr, A, K1, K0, g, ka), g_alpha, S2.sum(0), S1.sum(0)


def moments_grad(x, g_mean, g_var, rowptr):
    mean, _var = _stats(x, rowptr)
    n = torch.tensor([max(hi - lo, 1) for lo, hi in _spans(rowptr, x.shape[0])], dtype=x.dtype).view(-1, 1)
    return affine(x, rowptr, mean, 2 * g_var / n, g_mean / n)


# ---- the kernels' chains in fp32 numpy ---------------------------------------------------------------------------------------
def team_of(F, max_len):
    """(CL, W): channel lanes and wavefronts of the team that csrc/event_norm.hip runs for this width and hint."""
    return (1 if F == 1 else 4 if F <= 4 else 16), (16 if max_len >= KERNEL_LONG else 1)


def team_sum(terms, CL, W):
    """[F] fp32: the sum of terms [n, F] as a team forms it: entry lane ge adds the rows ge, ge + S, ... in ascending order
    from +0 (rows past the event add +0: no bit changes), the entry lanes of a wavefront combine by the xor butterfly, the
    wavefronts in order."""
    n, F = terms.shape
    EL = 64 // CL
    S = W * EL
    m = -(-n // S)
    buf = np.zeros((max(m, 1) * S, F), dtype=np.float32)
    buf[:n] = terms
    buf = buf.reshape(-1, S, F)
    acc = np.zeros((S, F), dtype=np.float32)
    for i in range(buf.shape[0]):
        acc = acc + buf[i]
    acc = acc.reshape(W, EL, F)
    off = EL // 2
    while off >= 1:
        acc = acc + acc[:, np.arange(EL) ^ off]
        off //= 2
    total = acc[0, 0]
    for w in range(1, W):
        total = total + acc[w, 0]
    return total


def emulate_moments(x, rowptr, max_len=0):
    x = np.asarray(x, dtype=np.float32)
    N, F = x.shape
    CL, W = team_of(F, max_len)
    B = len(rowptr) - 1
    mean, var = np.zeros((B, F), dtype=np.float32), np.zeros((B, F), dtype=np.float32)
    for b, (lo, hi) in enumerate(_spans(torch.as_tensor(rowptr), N)):
        if hi > lo:
            n = np.float32(hi - lo)
            mean[b] = team_sum(x[lo:hi], CL, W) / n
            d = x[lo:hi] - mean[b]
            var[b] = team_sum(d * d, CL, W) / n
    return mean, var


def emulate_dots(g, x, rowptr, shift=None, scale=None, max_len=0):
    g = np.asarray(g, dtype=np.float32)
    N, F = g.shape
    CL, W = team_of(F, max_len)
    B = len(rowptr) - 1
    s1 = np.zeros((B, F), dtype=np.float32)
    s2 = None if x is None else np.zeros((B, F), dtype=np.float32)
    for b, (lo, hi) in enumerate(_spans(torch.as_tensor(rowptr), N)):
        s1[b] = team_sum(g[lo:hi], CL, W)
        if x is not None:
            xh = (np.asarray(x[lo:hi], dtype=np.float32) - shift[b]) * scale[b]
            s2[b] = team_sum(g[lo:hi] * xh, CL, W)
    return s1, s2


class FakeKernels:
    """Stand-ins for deepmetv2_amd._native._event_moments / _event_dots / _event_affine on CPU tensors over the emulation."""

    def moments(self, x, rowptr, max_len=0):
        mean, var = emulate_moments(x.detach().numpy(), rowptr, max_len)
        return torch.from_numpy(mean), torch.from_numpy(var)

    def dots(self, g, x, rowptr, shift=None, scale=None, max_len=0):
        s1, s2 = emulate_dots(g.detach().numpy(), None if x is None else x.detach().numpy(), rowptr,
                              None if shift is None else shift.numpy(), None if scale is None else scale.numpy(), max_len)
        return torch.from_numpy(s1), None if s2 is None else torch.from_numpy(s2)

    def affine(self, x, rowptr, shift, k1, k0, g=None, ka=None):
        assert x.dtype == torch.float32 and all(t.shape == (rowptr.numel() - 1, x.shape[1]) for t in (shift, k1, k0))
        return affine(x.detach(), rowptr, shift, k1, k0, None if g is None else g.detach(), ka)

    def install(self, monkeypatch):
        import deepmetv2_amd._native as nat
        monkeypatch.setattr(nat, "_event_moments", self.moments)
        monkeypatch.setattr(nat, "_event_dots", self.dots)
        monkeypatch.setattr(nat, "_event_affine", self.affine)


# ---- torch_geometric.nn.norm as published, over a batch vector, in the dtype of x ----------------------------------------------
def _sum(x, batch, B):
    return torch.zeros((B, x.shape[1]), dtype=x.dtype).index_add(0, batch, x)


def _degree(batch, B, dtype):
    return torch.bincount(batch, minlength=B).to(dtype)


def up_graph_norm(x, batch, B, p, cfg):
    norm = _degree(batch, B, x.dtype).clamp(min=1).view(-1, 1)
    mean = _sum(x, batch, B) / norm
    out = x - mean.index_select(0, batch) * p["mean_scale"]
    var = _sum(out.pow(2), batch, B) / norm
    std = (var + cfg["eps"]).sqrt().index_select(0, batch)
    return p["weight"] * out / std + p["bias"]


def up_instance_stats(x, batch, B):
    """(mean, biased var, unbiased var) [B, F] as upstream's InstanceNorm forms them."""
    norm = _degree(batch, B, x.dtype).clamp(min=1).view(-1, 1)
    unbiased_norm = (norm - 1).clamp(min=1)
    mean = _sum(x, batch, B) / norm
    xc = x - mean.index_select(0, batch)
    var = _sum(xc * xc, batch, B)
    return mean, var / norm, var / unbiased_norm


def up_instance_norm(x, batch, B, p, cfg):
    if cfg.get("running") is not None:        # evaluation with tracked statistics
        mean, var = (t.view(1, -1).expand(B, -1) for t in cfg["running"])
    else:
        mean, var, _unbiased = up_instance_stats(x, batch, B)
    out = (x - mean.index_select(0, batch)) / (var + cfg["eps"]).sqrt().index_select(0, batch)
    if "weight" in p:
        out = out * p["weight"].view(1, -1) + p["bias"].view(1, -1)
    return out


def up_layer_norm(x, batch, B, p, cfg):
    if cfg.get("mode", "graph") == "node":
        return torch.nn.functional.layer_norm(x, (x.shape[1],), p.get("weight"), p.get("bias"), cfg["eps"])
    norm = (_degree(batch, B, x.dtype).clamp(min=1) * x.shape[1]).view(-1, 1)
    mean = _sum(x, batch, B).sum(-1, keepdim=True) / norm
    xc = x - mean.index_select(0, batch)
    var = _sum(xc * xc, batch, B).sum(-1, keepdim=True) / norm
    out = xc / (var + cfg["eps"]).sqrt().index_select(0, batch)
    if "weight" in p:
        out = out * p["weight"] + p["bias"]
    return out


def up_pair_norm(x, batch, B, p, cfg):
    norm = _degree(batch, B, x.dtype).clamp(min=1).view(-1, 1)
    xc = x - (_sum(x, batch, B) / norm).index_select(0, batch)
    if cfg.get("scale_individually"):
        return cfg["scale"] * xc / (cfg["eps"] + xc.norm(2, -1, keepdim=True))
    sq = _sum(xc.pow(2).sum(-1, keepdim=True), batch, B) / norm
    return cfg["scale"] * xc / (cfg["eps"] + sq).sqrt().index_select(0, batch)


def up_graph_size_norm(x, batch, B, p, cfg):
    return x / _degree(batch, B, x.dtype).sqrt().index_select(0, batch).view(-1, 1)


def up_mean_subtraction(x, batch, B, p, cfg):
    norm = _degree(batch, B, x.dtype).clamp(min=1).view(-1, 1)
    return x - (_sum(x, batch, B) / norm).index_select(0, batch)


# name: (the package's class, its constructor's options, the restatement, the restatement's settings)
LAYERS = {
    "graph_norm": ("GraphNorm", {}, up_graph_norm, {"eps": 1e-5}),
    "instance_norm": ("InstanceNorm", {}, up_instance_norm, {"eps": 1e-5}),
    "instance_norm_affine": ("InstanceNorm", {"affine": True, "eps": 1e-3}, up_instance_norm, {"eps": 1e-3}),
    "layer_norm": ("LayerNorm", {}, up_layer_norm, {"eps": 1e-5}),
    "layer_norm_plain": ("LayerNorm", {"affine": False}, up_layer_norm, {"eps": 1e-5}),
    "pair_norm": ("PairNorm", {"scale": 1.7}, up_pair_norm, {"eps": 1e-5, "scale": 1.7}),
    "pair_norm_individually": ("PairNorm", {"scale": 0.6, "scale_individually": True}, up_pair_norm,
                               {"eps": 1e-5, "scale": 0.6, "scale_individually": True}),
    "graph_size_norm": ("GraphSizeNorm", {}, up_graph_size_norm, {}),
    "mean_subtraction": ("MeanSubtractionNorm", {}, up_mean_subtraction, {}),
}
_NEEDS_CHANNELS = ("GraphNorm", "InstanceNorm", "LayerNorm")


def build_layer(name, F):
    """The package's layer with drawn (not ones and zeros) parameters."""
    import deepmetv2_amd as dm
    cls, kwargs, _up, _cfg = LAYERS[name]
    mod = getattr(dm, cls)(F, **kwargs) if cls in _NEEDS_CHANNELS else getattr(dm, cls)(**kwargs)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for pname, p in mod.named_parameters():
            p.copy_((0.0 if pname == "bias" else 1.0) + 0.3 * torch.randn(p.shape, generator=g))
    return mod


def layer_tensors_ours(mod, x, batch, g, batch_size=None):
    """[(name, tensor)]: out, g_x and every parameter's gradient of mod(x, batch) under the upstream gradient g."""
    xx = x.clone().requires_grad_(True)
    for p in mod.parameters():
        p.grad = None
    out = mod(xx, batch, batch_size)
    out.backward(g.to(out.device))
    return [("out", out.detach()), ("g_x", xx.grad)] + [(n, p.grad) for n, p in mod.named_parameters()]


def layer_tensors_upstream(name, mod, x, batch, B, g, dtype, running=None):
    _cls, _kwargs, up, cfg = LAYERS[name]
    cfg = dict(cfg, running=running)
    p = {n: t.detach().cpu().to(dtype).clone().requires_grad_(True) for n, t in mod.named_parameters()}
    xx = x.to(dtype).clone().requires_grad_(True)
    out = up(xx, batch, B, p, cfg)
    out.backward(g.to(dtype))
    return [("out", out.detach()), ("g_x", xx.grad)] + [(n, p[n].grad) for n, _ in mod.named_parameters()]

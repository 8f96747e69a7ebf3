"""Normalisation over the nodes of each event: GraphNorm, InstanceNorm, LayerNorm, PairNorm, GraphSizeNorm and
MeanSubtractionNorm of torch_geometric.nn.norm, and the two operators under them (csrc/event_norm.hip).

event_moments gives the per-event column mean and (biased) variance; event_normalize is one autograd Function around

    forward   event_moments -> arithmetic on the [B, F] statistics -> one elementwise pass (event_affine)
    backward  event_dots (the per-event sums of g and of g * xh) -> [B, F] arithmetic -> one elementwise pass with g

so the forward reads x twice (the second walk of the variance comes from L2) and writes y, and the backward makes two passes
over [N, F] and allocates nothing of that size but g_x.  The [B, F] arithmetic is torch on the device: no host sync.
The four Functions are `once_differentiable`: double backward raises.

Modes of event_normalize, per event b and channel c, with mu and var from event_moments and alpha = mean_scale:
    channel   A = alpha mu,  q = var + (1 - alpha)^2 mu^2   (= mean((x - alpha mu)^2): a sum of non-negatives; (1 - alpha) mu
              is evaluated as mu - A, from the rounded A that is subtracted from x)
    graph     A = mu_b = mean_c mu,  q_b = mean_c (var + (mu - mu_b)^2)           (LayerNorm over nodes and channels)
    pair      A = mu,  q_b = sum_c var                                             (PairNorm)
    y = (x - A) * (r w) + bias,  r = 1 / sqrt(q + eps)
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable
import torch.nn.functional as F_

from . import _native
from . import graph as _graph
from .scatter import _HALF, _csr_rowptr, _mean_len

_MODES = ("channel", "graph", "pair")


def _events(who: str, x: torch.Tensor, batch: Optional[torch.Tensor], ptr: Optional[torch.Tensor],
            batch_size: Optional[int]):
    """(rowptr int32 [B+1], max_len hint) of x's rows: `ptr` wins (clamped on the device, no sync), then a batch vector
    (graph.batch_info: no sync when registered, ValueError when unsorted or out of range), else one event."""
    if x.dim() != 2:
        raise ValueError(f"{who}: x must be [N, F], got {tuple(x.shape)}")
    if x.shape[1] < 1:
        raise ValueError(f"{who}: x must have at least one channel")
    if not x.dtype.is_floating_point or x.dtype == torch.float64:
        raise TypeError(f"{who}: x must be float32, bfloat16 or float16, got {x.dtype}")
    N = x.shape[0]
    if ptr is not None:
        return _csr_rowptr(ptr, N), _mean_len(N, ptr.numel() - 1)
    if batch is None:
        return torch.tensor([0, N], dtype=torch.int32, device=x.device), N
    info = _graph.batch_info(batch, N, x.device, batch_size)
    return _csr_rowptr(info.ptr, N), max(info.max_nodes or 0, _mean_len(N, info.num_events))


def _counts(rowptr: torch.Tensor) -> torch.Tensor:
    """[B, 1] float: the events' lengths as the kernels see them."""
    return rowptr.diff().clamp(min=0).to(torch.float32).view(-1, 1)


def _full(t: torch.Tensor, B: int, F: int) -> torch.Tensor:
    return t.expand(B, F).contiguous()


class _EventMoments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rowptr, max_len):
        mean, var = _native._event_moments(x, rowptr, max_len)
        ctx.save_for_backward(x, rowptr, mean)
        return mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mean, g_var):
        x, rowptr, mean = ctx.saved_tensors
        inv_n = 1.0 / _counts(rowptr).clamp(min=1.0)
        k1 = (2.0 * g_var.float()) * inv_n if g_var is not None else torch.zeros_like(mean)
        k0 = g_mean.float() * inv_n if g_mean is not None else torch.zeros_like(mean)
        return _native._event_affine(x, rowptr, mean, k1.contiguous(), k0.contiguous()), None, None


def event_moments(x: torch.Tensor, batch: Optional[torch.Tensor] = None, ptr: Optional[torch.Tensor] = None,
                  batch_size: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(mean [B, F], var [B, F], count [B]) of the rows of every event of x [N, F]: mean = fp32 sum / n, var = the mean of
    (x - mean)^2 taken in a second walk centred on the event's own mean (biased; never a difference of two means); an empty
    event gives 0 and 0.  Events come from `ptr` (it wins; clamped to [0, N], no host sync), a batch vector (no sync when
    registered) or neither (one event).  Differentiable in x: one elementwise launch.  bf16 / fp16 x is computed in fp32 and
    the statistics returned in x.dtype."""
    rowptr, max_len = _events("event_moments", x, batch, ptr, batch_size)
    mean, var = _EventMoments.apply(x.float(), rowptr, max_len)
    count = rowptr.diff().clamp(min=0).to(torch.int64)
    return (mean.to(x.dtype), var.to(x.dtype), count) if x.dtype in _HALF else (mean, var, count)


class _EventNormalize(torch.autograd.Function):
    """(y, mean, var); mean_scale and weight: a [F] tensor, a python float (not differentiated) or None (1)."""

    @staticmethod
    def forward(ctx, x, rowptr, max_len, mean_scale, weight, bias, eps, mode):
        N, F = x.shape
        B = rowptr.numel() - 1
        mean, var = _native._event_moments(x, rowptr, max_len)
        alpha = 1.0 if mean_scale is None else mean_scale
        plain = not torch.is_tensor(alpha) and float(alpha) == 1.0        # alpha = 1: A = mu and q = var, bit for bit
        if mode == "channel":
            # (1 - alpha) mu is taken as mu - A from the rounded A the kernel subtracts: q is then the mean of (x - A)^2
            # for that very A, and a one-node event (x = mu) normalises to xh^2 = q / (q + eps) to the last bits
            A = mean if plain else mean * alpha
            q = var if plain else var + (mean - A) ** 2
        elif mode == "graph":
            m = mean.mean(1, keepdim=True)
            A = m
            q = (var + (mean - m) ** 2).mean(1, keepdim=True)
        else:
            A = mean
            q = var.sum(1, keepdim=True)
        r = 1.0 / torch.sqrt(q + eps)
        A, r = _full(A, B, F), _full(r, B, F)
        k1 = r if weight is None else _full(r * weight, B, F)
        k0 = torch.zeros_like(k1) if bias is None else _full(bias.view(1, F), B, F)
        y = _native._event_affine(x, rowptr, A, k1, k0)
        ctx.save_for_backward(x, rowptr, mean, A, r, k1, *(t for t in (mean_scale, weight) if torch.is_tensor(t)))
        ctx.cfg = (max_len, mode, torch.is_tensor(mean_scale), torch.is_tensor(weight),
                   None if torch.is_tensor(mean_scale) else alpha, None if torch.is_tensor(weight) else weight)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_mean, _g_var):
        x, rowptr, mean, A, r, ka, *rest = ctx.saved_tensors
        max_len, mode, t_alpha, t_weight, alpha, weight = ctx.cfg
        if t_alpha:
            alpha, rest = rest[0], rest[1:]
        if t_weight:
            weight = rest[0]
        need_x, need_alpha, need_w, need_b = (ctx.needs_input_grad[i] for i in (0, 3, 4, 5))
        if not (need_x or need_alpha or need_w or need_b):
            return (None,) * 8
        g = g.float()
        B, F = mean.shape
        S1, S2 = _native._event_dots(g, x, rowptr, A, r, max_len)
        g_x = g_alpha = None
        inv_n = 1.0 / _counts(rowptr).clamp(min=1.0)
        w = 1.0 if weight is None else weight
        if mode == "channel":
            plain = not t_alpha and float(alpha) == 1.0
            t = ka * r * S2
            G = ka * S1 if plain else ka * S1 - t * (mean - A)          # (1 - alpha) mu, as the forward takes it
            K1, K0 = -(t * inv_n), -((G if plain else alpha * G) * inv_n)
            if need_alpha:
                g_alpha = -(mean * G).sum(0)
        elif mode == "graph":
            T1, T2 = (w * S1).sum(1, keepdim=True), (w * S2).sum(1, keepdim=True)
            K1 = _full(-(r[:, :1] * r[:, :1] * T2) * inv_n / F, B, F)
            K0 = _full(-(r[:, :1] * T1) * inv_n / F, B, F)
        else:
            T2 = (w * S2).sum(1, keepdim=True)
            K1 = _full(-(r[:, :1] * r[:, :1] * T2) * inv_n, B, F)
            K0 = -(ka * S1) * inv_n
        if need_x:
            g_x = _native._event_affine(x, rowptr, A, K1.contiguous(), K0.contiguous(), g, ka)
        return (g_x, None, None, g_alpha, S2.sum(0) if need_w else None, S1.sum(0) if need_b else None, None, None)


def _normalize(who, x, batch, ptr, batch_size, mean_scale, weight, bias, eps, mode):
    if mode not in _MODES:
        raise ValueError(f"{who}: unknown mode {mode!r} (one of {_MODES})")
    rowptr, max_len = _events(who, x, batch, ptr, batch_size)
    C = x.shape[1]
    for name, t in (("mean_scale", mean_scale), ("weight", weight), ("bias", bias)):
        if torch.is_tensor(t) and (t.dim() != 1 or t.numel() != C):
            raise ValueError(f"{who}: {name} must have {C} elements, got {tuple(t.shape)}")
    if mode != "channel" and mean_scale is not None:
        raise ValueError(f"{who}: mean_scale goes with mode='channel'")
    f32 = lambda t: t.float() if torch.is_tensor(t) else t      # noqa: E731
    y, mean, var = _EventNormalize.apply(x.float(), rowptr, max_len, f32(mean_scale), f32(weight), f32(bias), float(eps),
                                         mode)
    return y.to(x.dtype), mean, var, rowptr


def event_normalize(x: torch.Tensor, batch: Optional[torch.Tensor] = None, ptr: Optional[torch.Tensor] = None,
                    batch_size: Optional[int] = None, mean_scale: Optional[torch.Tensor] = None,
                    weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, eps: float = 1e-5,
                    mode: str = "channel") -> torch.Tensor:
    """y = (x - A) * (r * weight) + bias over the nodes of every event of x [N, F], r = 1 / sqrt(q + eps), with A and q from
    the event's own statistics as `mode` says (the module docstring): 'channel' (GraphNorm; mean_scale = alpha, None = 1:
    InstanceNorm), 'graph' (LayerNorm over all nodes and channels of an event), 'pair' (PairNorm).  One autograd Function,
    differentiable in x, mean_scale, weight and bias; events as in event_moments.  bf16 / fp16 x is computed in fp32 and
    returned in x.dtype.  Rows that no event of `ptr` owns come back as zeros."""
    return _normalize("event_normalize", x, batch, ptr, batch_size, mean_scale, weight, bias, eps, mode)[0]


class _EventAffine(torch.autograd.Function):
    """out = (x - shift[b]) * k1[b] + k0[b] with [B, F] operands; differentiable in all four."""

    @staticmethod
    def forward(ctx, x, rowptr, max_len, shift, k1, k0):
        ctx.save_for_backward(x, rowptr, shift, k1)
        ctx.max_len = max_len
        return _native._event_affine(x, rowptr, shift, k1, k0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, rowptr, shift, k1 = ctx.saved_tensors
        need_x, _r, _m, need_shift, need_k1, need_k0 = ctx.needs_input_grad
        g = g.float()
        zero = torch.zeros_like(k1)
        g_x = _native._event_affine(g, rowptr, zero, k1, zero) if need_x else None
        S1 = S2 = None
        if need_k1:
            S1, S2 = _native._event_dots(g, x, rowptr, shift, torch.ones_like(k1), ctx.max_len)
        elif need_shift or need_k0:
            S1, _ = _native._event_dots(g, None, rowptr, max_len=ctx.max_len)
        return g_x, None, None, -(k1 * S1) if need_shift else None, S2 if need_k1 else None, S1 if need_k0 else None


class _Center(torch.autograd.Function):
    """x - mu[b]: the statistics and one elementwise launch forward, the sums of g and one elementwise launch backward."""

    @staticmethod
    def forward(ctx, x, rowptr, max_len):
        mean, _var = _native._event_moments(x, rowptr, max_len)
        ctx.save_for_backward(rowptr)
        ctx.max_len = max_len
        return _native._event_affine(x, rowptr, mean, torch.ones_like(mean), torch.zeros_like(mean))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (rowptr,) = ctx.saved_tensors
        g = g.float()
        S1, _ = _native._event_dots(g, None, rowptr, max_len=ctx.max_len)
        shift = S1 / _counts(rowptr).clamp(min=1.0)
        return _native._event_affine(g, rowptr, shift, torch.ones_like(shift), torch.zeros_like(shift)), None, None


# ---- the layers of torch_geometric.nn.norm ----------------------------------------------------------------------------------
class GraphNorm(torch.nn.Module):
    """torch_geometric.nn.GraphNorm: weight * (x - mean_scale * mu) / sqrt(mean((x - mean_scale * mu)^2) + eps) + bias
    over the nodes of every graph, per channel."""

    def __init__(self, in_channels: int, eps: float = 1e-5):
        super().__init__()
        self.in_channels = in_channels
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(in_channels))
        self.bias = torch.nn.Parameter(torch.zeros(in_channels))
        self.mean_scale = torch.nn.Parameter(torch.ones(in_channels))
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)
        torch.nn.init.zeros_(self.bias)
        torch.nn.init.ones_(self.mean_scale)

    def forward(self, x: torch.Tensor, batch: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> torch.Tensor:
        return _normalize("GraphNorm", x, batch, None, batch_size, self.mean_scale, self.weight, self.bias, self.eps,
                          "channel")[0]

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels})"


class InstanceNorm(torch.nn.modules.instancenorm._InstanceNorm):
    """torch_geometric.nn.InstanceNorm: (x - mu) / sqrt(var + eps) per graph and channel, then the optional affine.  With
    track_running_stats the buffers follow upstream: the mean over the graphs of the batch of the per-graph mean and of the
    unbiased variance (divisor max(n - 1, 1)); evaluation then normalises with the buffers."""

    def __init__(self, in_channels: int, eps: float = 1e-5, momentum: float = 0.1, affine: bool = False,
                 track_running_stats: bool = False):
        super().__init__(in_channels, eps, momentum, affine, track_running_stats)

    def forward(self, x: torch.Tensor, batch: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> torch.Tensor:
        if self.training or not self.track_running_stats:
            y, mean, var, rowptr = _normalize("InstanceNorm", x, batch, None, batch_size, None, self.weight, self.bias,
                                              self.eps, "channel")
            if self.track_running_stats and self.training:
                with torch.no_grad():
                    n = _counts(rowptr)
                    unbiased = var * (n / (n - 1.0).clamp(min=1.0))
                    m = self.momentum
                    self.running_mean.mul_(1 - m).add_(m * mean.mean(0))
                    self.running_var.mul_(1 - m).add_(m * unbiased.mean(0))
            return y
        rowptr, max_len = _events("InstanceNorm", x, batch, None, batch_size)
        B, C = rowptr.numel() - 1, x.shape[1]
        k1 = 1.0 / torch.sqrt(self.running_var.float() + self.eps)
        if self.weight is not None:
            k1 = k1 * self.weight.float()
        k0 = torch.zeros_like(k1) if self.bias is None else self.bias.float()
        y = _EventAffine.apply(x.float(), rowptr, max_len, _full(self.running_mean.float().view(1, C), B, C),
                               _full(k1.view(1, C), B, C), _full(k0.view(1, C), B, C))
        return y.to(x.dtype)

    def _check_input_dim(self, input):
        if input.dim() != 2:
            raise ValueError(f"InstanceNorm: x must be [N, F], got {tuple(input.shape)}")

    def __repr__(self):
        return f"{self.__class__.__name__}({self.num_features})"


class LayerNorm(torch.nn.Module):
    """torch_geometric.nn.LayerNorm: mode='graph' normalises over all nodes and channels of every graph (batch None: the
    whole input is one graph), mode='node' is torch.nn.functional.layer_norm over the channels of every node."""

    def __init__(self, in_channels: int, eps: float = 1e-5, affine: bool = True, mode: str = "graph"):
        super().__init__()
        if mode not in ("graph", "node"):
            raise ValueError(f"LayerNorm: unknown mode {mode!r} ('graph' or 'node')")
        self.in_channels = in_channels
        self.eps = eps
        self.affine = affine
        self.mode = mode
        if affine:
            self.weight = torch.nn.Parameter(torch.ones(in_channels))
            self.bias = torch.nn.Parameter(torch.zeros(in_channels))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.affine:
            torch.nn.init.ones_(self.weight)
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: torch.Tensor, batch: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> torch.Tensor:
        if self.mode == "node":
            return F_.layer_norm(x, (self.in_channels,), self.weight, self.bias, self.eps)
        return _normalize("LayerNorm", x, batch, None, batch_size, None, self.weight, self.bias, self.eps, "graph")[0]

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, affine={self.affine}, mode={self.mode})"


class PairNorm(torch.nn.Module):
    """torch_geometric.nn.PairNorm: x_c = x - mu per graph, then scale * x_c / sqrt(eps + mean_n |x_c[n]|^2), or with
    scale_individually scale * x_c / (eps + |x_c[n]|) per node (the centring by the kernels, the row norms in torch)."""

    def __init__(self, scale: float = 1.0, scale_individually: bool = False, eps: float = 1e-5):
        super().__init__()
        self.scale = scale
        self.scale_individually = scale_individually
        self.eps = eps

    def forward(self, x: torch.Tensor, batch: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> torch.Tensor:
        if not self.scale_individually:
            return _normalize("PairNorm", x, batch, None, batch_size, None, float(self.scale), None, self.eps, "pair")[0]
        rowptr, max_len = _events("PairNorm", x, batch, None, batch_size)
        xc = _Center.apply(x.float(), rowptr, max_len).to(x.dtype)
        return self.scale * xc / (self.eps + xc.norm(2, -1, keepdim=True))

    def __repr__(self):
        return f"{self.__class__.__name__}()"


class GraphSizeNorm(torch.nn.Module):
    """torch_geometric.nn.GraphSizeNorm: x / sqrt(n_b), as one elementwise launch (x * fp32(1 / sqrt(n_b)))."""

    def forward(self, x: torch.Tensor, batch: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> torch.Tensor:
        rowptr, max_len = _events("GraphSizeNorm", x, batch, None, batch_size)
        B, C = rowptr.numel() - 1, x.shape[1]
        k1 = _full(1.0 / torch.sqrt(_counts(rowptr).clamp(min=1.0)), B, C)
        zero = torch.zeros_like(k1)
        return _EventAffine.apply(x.float(), rowptr, max_len, zero, k1, zero).to(x.dtype)

    def __repr__(self):
        return f"{self.__class__.__name__}()"


class MeanSubtractionNorm(torch.nn.Module):
    """torch_geometric.nn.MeanSubtractionNorm: x - mu per graph and channel."""

    def forward(self, x: torch.Tensor, batch: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> torch.Tensor:
        rowptr, max_len = _events("MeanSubtractionNorm", x, batch, None, batch_size)
        return _Center.apply(x.float(), rowptr, max_len).to(x.dtype)

    def reset_parameters(self):
        pass

    def __repr__(self):
        return f"{self.__class__.__name__}()"

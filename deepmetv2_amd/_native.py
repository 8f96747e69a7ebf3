"""Tensor-level wrappers over the C ABI: validate, allocate outputs / workspace from torch's caching allocator,
enqueue on the current HIP stream.  PyTorch is used here for device memory and streams only.

Every function requires ROCm device tensors and raises otherwise -- there is no CPU path in the product.
"""
from __future__ import annotations

import contextlib
import ctypes
import inspect
import math
import os
from typing import Optional, Tuple

import torch

from . import _lib


def _require_device(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                "deepmetv2_amd: operator called with a non-GPU tensor. The HIP extension is the only "
                "implementation (no CPU fallback); move inputs to a ROCm device.")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("deepmetv2_amd: all tensors must live on the same device")
    return dev


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev: torch.device) -> int:
    """The raw hipStream_t of torch's current stream on `dev` (one C call: torch.cuda.current_stream() builds a Stream object
    first -- 5 us each, ~13 times per training step on the launch thread)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


_NULL_CTX = contextlib.nullcontext()


def _on(dev: torch.device):
    """Context that makes `dev` the current device for a native call -- a no-op object when it already is (the usual
    case: one process per GPU): entering torch.cuda.device() costs the launch thread several microseconds per call,
    ~70 times per training step."""
    if dev.index is None or torch.cuda.current_device() == dev.index:
        return _NULL_CTX
    return torch.cuda.device(dev)


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """`t` itself when its storage starts on a 16-byte boundary, else a fresh (aligned) copy.  The kernels read rows and
    per-channel vectors as float4; a contiguous tensor that is a view into somebody else's flat buffer may start anywhere."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _f32a(t: torch.Tensor, name: str) -> torch.Tensor:
    """_f32c, then _aligned16: what an entry asks of an operand its kernel reads as float4."""
    return _aligned16(_f32c(t, name))


def no_double_backward(who: str) -> None:
    """First line of a backward that runs native kernels and is on the launch thread of the training step.  Grad mode is on
    inside a backward only under create_graph=True; the gradients returned here would carry no grad_fn and a second
    derivative through them would silently treat them as constants.  (`once_differentiable` does the same with one more
    Python frame and a no_grad block per call.)"""
    if torch.is_grad_enabled():
        raise RuntimeError(f"{who}: double backward is not supported: the backward runs native kernels and is "
                           f"once_differentiable (differentiating it with create_graph=True would give constants)")


def _ptr(t: Optional[torch.Tensor]):
    """The address of an optional tensor: None (a null pointer) for None and for an empty tensor."""
    return t.data_ptr() if t is not None and t.numel() else None


def _bn_affine_operands(who: str, raw: torch.Tensor, residual: Optional[torch.Tensor], gamma: torch.Tensor,
                        beta: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor):
    """The operands of y = residual + BatchNorm(raw) with the statistics given, for every entry that applies or carries the
    transform (csrc/bn_affine.h): detached contiguous fp32, residual of raw's shape, four vectors of raw.shape[1] elements.
    Returns (raw, residual or None, [gamma, beta, mean, invstd], whether all of them start on a 16-byte boundary)."""
    raw = _f32c(raw.detach(), "raw")
    if raw.dim() != 2:
        raise ValueError(f"{who}: raw must be 2-D [N, H], got {tuple(raw.shape)}")
    if residual is not None:
        residual = _f32c(residual.detach(), "residual")
        if residual.shape != raw.shape:
            raise ValueError(f"{who}: residual must have the shape of raw")
    vec = [_f32c(t.detach(), n) for t, n in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (invstd, "invstd"))]
    if any(v.numel() != raw.shape[1] for v in vec):
        raise ValueError(f"{who}: gamma / beta / mean / invstd must have H elements")
    aligned = not any(t.data_ptr() % 16 for t in (raw, *vec, *(() if residual is None else (residual,))))
    return raw, residual, vec, aligned


def _pq_tables(N: int, sliced, dev: torch.device):
    """The outputs of a node-level dense layer 32 -> 32 that another launch carries: (P, Q, layout code of the C ABI,
    `sliced` as gather_max takes it) -- fp32 [N, 32] (0), fp32 slice-major [4, N, 8] (1), or for sliced == "bf16" P fp32 and
    Q bf16, both [N, 32] (2: node_linear_split_bf16)."""
    if sliced == "bf16":
        return (torch.empty((N, 32), dtype=torch.float32, device=dev), torch.empty((N, 32), dtype=torch.bfloat16, device=dev),
                2, sliced)
    PQ = torch.empty((2, 4, N, 8) if sliced else (2, N, 32), dtype=torch.float32, device=dev)
    return PQ[0], PQ[1], (1 if sliced else 0), bool(sliced)


def _ws(nbytes: int, dev: torch.device) -> torch.Tensor:
    return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=dev)


class KernelTimer:
    """Optional HIP-event bracket around named native calls, recorded on the stream the kernel is launched on
    (bench.py turns it on for the roofline figure; costs two event records per call, no synchronisation)."""

    def __init__(self):
        self.enabled = False
        self.only = None        # optional set of names: bracket just these (every bracket costs two stream commands)
        self._pending = {}

    def reset(self) -> None:
        self._pending = {}

    def record(self, name: str, dev: torch.device):
        if not self.enabled or (self.only is not None and name not in self.only):
            return None
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream(dev))
        self._pending.setdefault(name, []).append((a, b))
        return b

    def calibrate(self, dev: torch.device, n: int = 50) -> float:
        """Cost of an EMPTY bracket (two event records back to back on the stream), in ms: the two records are
        stream commands of their own, so a bracket reads ~2-4 us longer than the kernel inside it."""
        pairs = []
        st = torch.cuda.current_stream(dev)
        for _ in range(n):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(st)
            b.record(st)
            pairs.append((a, b))
        torch.cuda.synchronize(dev)
        ts = sorted(a.elapsed_time(b) for a, b in pairs)
        self.overhead_ms = ts[len(ts) // 2]
        return self.overhead_ms

    def summary(self) -> dict:
        """{name: (launches, mean_ms)} with the empty-bracket cost removed -- call after a device synchronise."""
        out = {}
        oh = getattr(self, "overhead_ms", 0.0)
        for name, pairs in self._pending.items():
            ts = [max(a.elapsed_time(b) - oh, 0.0) for a, b in pairs]
            out[name] = (len(ts), sum(ts) / max(len(ts), 1))
        return out


timer = KernelTimer()

# which gather + max kernel the last gather_max* call launched (bench.py labels its roofline block with it)
last_gather_kernel = None

# gather+max kernel form: "auto" = LDS-resident when the caller says the events fit, else L2 gathers;
# "lds" / "l2-only" force one form (experiments, tools/gather_micro.py)
GATHER_MAX_FORM = os.environ.get("DMET_GATHER_MAX_FORM", "auto")
RADIUS_FORM = os.environ.get("DMET_RADIUS", "windowed")   # "sweep": all pairs of an event (dmet_radius_f32)


# table widths the LDS-resident fp32 gather kernels are built for (k = 4 K4; 20 = the reference's own default,
# model/graph_met_network.py:63); other widths take the L2 form
LDS_GATHER_K = (8, 16, 20, 32)


def _note_gather(name: str) -> None:
    global last_gather_kernel
    last_gather_kernel = name


# ---- K1 ------------------------------------------------------------------------------------------------------
# ---- the weight-gradient sums of a backward pass in one launch (dmet_finalize_defer_begin / dmet_finalize_flush) --------
DEFER_FINALIZE = os.environ.get("DMET_DEFER_FINALIZE", "1") != "0"
_DEFER = {"active": False, "keep": [], "dev": None, "seen": set()}


def finalize_defer_begin() -> bool:
    """From here to finalize_flush() (process-wide: autograd runs backward on a thread of its own) edgeconv_linear_bwd, encode_bwd / encode_bn_bwd and head_bwd leave
    the small second launch that sums their weight-gradient partials to ONE launch at the flush: their parameter
    gradients hold garbage until then (the harness flushes right after loss.backward()).  Kept alive here until the flush:
    the calls' workspaces AND the memory of the gradients they returned -- autograd drops the gradient of a parameter
    with requires_grad=False during the pass, and the flush would write into whoever got the block next.  The queue of
    the library holds 8 sums; a call beyond them sums at once.  DMET_DEFER_FINALIZE=0: a no-op (every call sums its own
    partials at once, as without this call).

    What the caller still has to hold to: nothing may READ one of those gradients before the flush.  Autograd itself
    does when a parameter is used twice in the pass (it adds the two gradients): the second call on the same
    parameters therefore forms the sums queued so far and its own at once (_defer_second_use).  Not covered: a weight that
    is no leaf (its gradient flows on into other backward nodes), tensor hooks on these parameters, a backward pass
    that accumulates into a .grad that is already there (train_step drops every .grad first)."""
    if not DEFER_FINALIZE:
        return False
    if _DEFER["active"]:
        finalize_flush()     # a deferral somebody left open (an exception between begin and flush): its sums are formed first
    _lib.check(_lib.load().dmet_finalize_defer_begin(), "dmet_finalize_defer_begin")
    _DEFER["active"], _DEFER["keep"], _DEFER["dev"], _DEFER["seen"] = True, [], None, set()
    return True


def finalize_flush() -> None:
    """Form every queued weight-gradient sum (one launch on the stream of the device the queued calls ran on) and end
    the deferral; a no-op outside one."""
    if not _DEFER["active"]:
        return
    dev = _DEFER["dev"]
    L = _lib.load()
    try:
        if dev is not None and L.dmet_finalize_pending() > 0:
            with _on(dev):
                _lib.check(L.dmet_finalize_flush(_stream(dev)), "dmet_finalize_flush")
        else:
            _lib.check(L.dmet_finalize_flush(None), "dmet_finalize_flush")
    finally:
        _DEFER["active"], _DEFER["keep"], _DEFER["dev"], _DEFER["seen"] = False, [], None, set()


def _defer_keep(dev: torch.device, ws: torch.Tensor, *outs: Optional[torch.Tensor]) -> None:
    """A queued sum reads its partials from the call's workspace `ws` at the flush and writes the gradients `outs` there:
    neither may go back to the allocator before.  Of the gradients the STORAGE is kept, not the tensor: a second
    reference to the tensor itself would make autograd copy it (unwritten) into .grad instead of taking it over."""
    if _DEFER["active"]:
        _DEFER["dev"] = dev
        _DEFER["keep"].append(ws)
        _DEFER["keep"].extend(t.untyped_storage() for t in outs if t is not None)


def _defer_second_use(dev: torch.device, *params: Optional[torch.Tensor]) -> bool:
    """Before a call that would queue the gradient sums of `params`: False when none of them was seen in this deferral
    (they are now).  A module applied twice comes here a second time: autograd adds the two gradients of a parameter as
    soon as it has both, so neither may be unwritten then.  The sums queued so far are formed now, in their queue order,
    and the library's queue is closed, so that the call sums at once; True -- the caller reopens it after the call
    (_defer_resume) for what the pass has left.  The bits are those of the per-call sums either way."""
    if not _DEFER["active"]:
        return False
    keys = {p.data_ptr() for p in params if p is not None}
    if _DEFER["seen"].isdisjoint(keys):
        _DEFER["seen"] |= keys
        return False
    L = _lib.load()
    qdev = _DEFER["dev"] if _DEFER["dev"] is not None else dev
    if L.dmet_finalize_pending() > 0:
        with _on(qdev):
            _lib.check(L.dmet_finalize_flush(_stream(qdev)), "dmet_finalize_flush")
    else:
        _lib.check(L.dmet_finalize_flush(None), "dmet_finalize_flush")
    return True


def _defer_resume() -> None:
    _lib.check(_lib.load().dmet_finalize_defer_begin(), "dmet_finalize_defer_begin")


def knn_size_hint(min_nodes: Optional[int], max_nodes: Optional[int]) -> None:
    """Tell the NEXT kNN build on this thread what the caller knows about its event sizes (dmet_knn_size_hint)."""
    if min_nodes and max_nodes:
        _lib.check(_lib.load().dmet_knn_size_hint(int(min_nodes), int(max_nodes)), "dmet_knn_size_hint")


def _knn_operands(x: torch.Tensor, ptr: torch.Tensor):
    """The checks of a one-set build: (dev, x as contiguous fp32, N, D, B)."""
    dev = _require_device(x, ptr)
    x = _f32c(x.detach(), "x")
    if x.dim() != 2:
        raise ValueError(f"x must be 2-D [N, D], got {tuple(x.shape)}")
    return (dev, x, *x.shape, ptr.numel() - 1)


def _knn_run(dev: torch.device, Nq: int, k: int, want_local: bool, ws_bytes: int, call):
    """The tables of a build over Nq queries and its workspace; call(nbr, dist, loc pointer or None, ws) runs on dev
    inside the 'knn' timer bracket.  Returns (nbr, dist, loc, ws, what call returned)."""
    nbr = torch.empty((Nq, k), dtype=torch.int32, device=dev)
    dist = torch.empty((Nq, k), dtype=torch.float32, device=dev)
    # uint16 payload in an int16 tensor (torch has no arithmetic on uint16; the kernels only reinterpret the bytes)
    loc = torch.empty((Nq, k), dtype=torch.int16, device=dev) if want_local else None
    ws = _ws(ws_bytes, dev)
    _t = timer.record('knn', dev)
    with _on(dev):
        extra = call(nbr, dist, _ptr(loc), ws)
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return nbr, dist, loc, ws, extra


def _knn(x: torch.Tensor, ptr: torch.Tensor, k: int, stats: Optional[dict], want_local: bool, dense=None):
    """dense = (W[32,64], b or None, sliced): also ask the build for the node-level dense layer of the EdgeConv that
    consumes the graph (dmet_knn_local_dense_f32); a fourth result (P, Q) or None is then returned."""
    dev, x, N, D, B = _knn_operands(x, ptr)
    L = _lib.load()
    asked = dense is not None
    if dense is not None and (D != 32 or N == 0 or B == 0 or tuple(dense[0].shape) != (32, 64)):
        dense = None

    def call(nbr, dist, loc_p, ws):     # -> (P, Q, sliced) if the build carried the dense layer, else None
        if dense is None:
            _lib.check(L.dmet_knn_local_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, k, nbr.data_ptr(), dist.data_ptr(),
                                            loc_p, ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_knn_local_f32")
            return None
        W, b, sliced = dense            # sliced: False / True, or "bf16" (P fp32, Q bf16: node_linear_split_bf16)
        W = _f32c(W.detach(), "W")
        b = _f32c(b.detach(), "b") if b is not None else None
        Pt, Qt, layout, sliced = _pq_tables(N, sliced, dev)
        done = ctypes.c_int(0)
        _lib.check(L.dmet_knn_local_dense_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, k, nbr.data_ptr(),
                                              dist.data_ptr(), loc_p, W.data_ptr(), _ptr(b), layout, Pt.data_ptr(),
                                              Qt.data_ptr(), ctypes.cast(ctypes.pointer(done), ctypes.c_void_p),
                                              ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_knn_local_dense_f32")
        return (Pt, Qt, sliced) if done.value else None

    nbr, dist, loc, ws, pq = _knn_run(dev, N, k, want_local, L.dmet_knn_workspace_bytes(N, B, D, k), call)
    if stats is not None and N > 0 and B > 0:
        with _on(dev):
            out = (ctypes.c_int64 * 2)()
            _lib.check(L.dmet_knn_fallback_stats(ws.data_ptr(), N, B, D, k, ctypes.cast(out, ctypes.c_void_p),
                                                 _stream(dev)), "dmet_knn_fallback_stats")
            stats["flagged_tiles"], stats["flagged_queries"] = int(out[0]), int(out[1])
            stats["tiles"] = (N + 127) // 128
            _lib.check(L.dmet_knn_retry_stats(ws.data_ptr(), N, B, D, k, ctypes.cast(out, ctypes.c_void_p),
                                              _stream(dev)), "dmet_knn_retry_stats")
            stats["second_attempts"], stats["second_attempt_queries"] = int(out[0]), int(out[1])
    if asked:
        return nbr, dist, loc, pq
    return nbr, dist, loc


def knn(x: torch.Tensor, ptr: torch.Tensor, k: int, stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """nbr[N,k] int32 (global ids, -1 padded), dist[N,k] fp32.  With a `stats` dict the call synchronises and stores
    stats['flagged_tiles'] / stats['flagged_queries'] (what the matrix-core path could not certify and recomputed
    exactly) and stats['second_attempts'] / stats['second_attempt_queries'] (wavefronts of the filter that swept their
    event a second time, and the queries they did it for); diagnostics only."""
    nbr, dist, _ = _knn(x, ptr, k, stats, False)
    return nbr, dist


def knn_local_dense(x: torch.Tensor, ptr: torch.Tensor, k: int, W: torch.Tensor, b: Optional[torch.Tensor],
                    sliced, stats: Optional[dict] = None):
    """knn_local() for the DynamicEdgeConv call shape: (nbr, dist, loc, pq) with pq = (P, Q, sliced) -- the node-level
    dense layer of node_linear_split(x, W, b, sliced) (sliced = "bf16": of node_linear_split_bf16(x, W, b)), computed by
    trailing workgroups of the build's filter launch -- or pq = None when this build took a path that cannot carry it
    (the caller then runs the dense layer itself)."""
    out = _knn(x, ptr, k, stats, True, dense=(W, b, sliced))
    return out if len(out) == 4 else (*out, None)


def knn_local(x: torch.Tensor, ptr: torch.Tensor, k: int, stats: Optional[dict] = None
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """knn() plus the same table as event-local uint16 ids (0xFFFF = empty slot; stored in an int16 tensor), written
    by the same kernels: half the id bytes for the LDS gather kernel.  Rows of events with more than 65535 nodes are
    unspecified (those events never take the LDS path)."""
    return _knn(x, ptr, k, stats, True)


def _period_array(period, D: int):
    """(host float array kept alive by the caller, its address) for a `period` of D floats, or (None, None)."""
    if period is None:
        return None, None
    if len(period) != D:
        raise ValueError(f"period has {len(period)} entries for {D} coordinates")
    per = (ctypes.c_float * D)(*[float(p) for p in period])    # host array, read by the C entry before it returns
    return per, ctypes.cast(per, ctypes.c_void_p)


def knn_periodic(x: torch.Tensor, ptr: torch.Tensor, k: int, period, want_local: bool):
    """knn() / knn_local() with periodic coordinates (dmet_knn_periodic_f32): period = D floats, period[c] > 0 the
    circumference of coordinate c, 0 a plain coordinate; D <= 8.  Returns (nbr, dist, loc), loc None unless
    want_local."""
    dev, x, N, D, B = _knn_operands(x, ptr)
    L = _lib.load()
    _per, per_p = _period_array(period, D)

    def call(nbr, dist, loc_p, ws):
        _lib.check(L.dmet_knn_periodic_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, k, per_p, nbr.data_ptr(),
                                           dist.data_ptr(), loc_p, ws.data_ptr(), ws.numel(), _stream(dev)),
                   "dmet_knn_periodic_f32")
    return _knn_run(dev, N, k, want_local, L.dmet_knn_workspace_bytes(N, B, D, k), call)[:3]


def _xy_operands(x: torch.Tensor, ptr_x: torch.Tensor, y: torch.Tensor, ptr_y: torch.Tensor):
    dev = _require_device(x, ptr_x, y, ptr_y)
    x = _f32c(x.detach(), "x")
    y = _f32c(y.detach(), "y")
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise ValueError(f"x and y must be [Nx, D] and [Ny, D], got {tuple(x.shape)} and {tuple(y.shape)}")
    if ptr_x.numel() != ptr_y.numel() or ptr_x.dtype != torch.int64 or ptr_y.dtype != torch.int64:
        raise ValueError("ptr_x and ptr_y must be int64 vectors over the same events")
    return dev, x, y, ptr_x.contiguous(), ptr_y.contiguous()


def knn_xy(x: torch.Tensor, ptr_x: torch.Tensor, y: torch.Tensor, ptr_y: torch.Tensor, k: int, period=None):
    """Two point sets (dmet_knn_xy_f32): for every row of y the k nearest rows of x of the same event.  nbr[Ny,k] int32
    (global x ids, -1 padded), dist[Ny,k] fp32 (1e10 padded).  period: None, or D floats as knn_periodic (D <= 8)."""
    dev, x, y, ptr_x, ptr_y = _xy_operands(x, ptr_x, y, ptr_y)
    L = _lib.load()
    (Nx, D), Ny, B = x.shape, y.shape[0], ptr_y.numel() - 1
    _per, per_p = _period_array(period, D)

    def call(nbr, dist, _loc_p, ws):
        _lib.check(L.dmet_knn_xy_f32(x.data_ptr(), ptr_x.data_ptr(), Nx, y.data_ptr(), ptr_y.data_ptr(), Ny, B, D, k, per_p,
                                     nbr.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                   "dmet_knn_xy_f32")
    return _knn_run(dev, Ny, k, False, L.dmet_knn_xy_workspace_bytes(Nx, Ny, B, D, k), call)[:2]


def _radius_build(x: torch.Tensor, ptr: torch.Tensor, r: float, max_nbr: int, skip_self: bool, pad: bool, local: bool,
                  int32_rows: bool, period, query=None):
    """One radius build: (nbr[N,max_nbr] int32 or None, cnt[N] int32, rows16 or None) over the N query rows -- the rows
    of x, or of y for query = (y, ptr_y) with x / ptr the candidates.  Picks the form and the one C entry of the request."""
    if query is None:
        dev, x, N, D, B = _knn_operands(x, ptr)
    else:
        dev, x, y, ptr, ptr_y = _xy_operands(x, ptr, *query)
        (Nx, D), N, B = x.shape, y.shape[0], ptr_y.numel() - 1
    L = _lib.load()
    per, per_p = _period_array(period, D)
    # the window runs on coordinate 0 of one point set; everything else is all pairs of an event (A/B and fallback)
    windowed = RADIUS_FORM != "sweep" and query is None and (per is None or per[0] == 0.0)
    skip32 = local and windowed and not int32_rows and not pad
    nbr = None if skip32 else torch.empty((N, max_nbr), dtype=torch.int32, device=dev)
    cnt = torch.empty((N,), dtype=torch.int32, device=dev)
    stride16 = (max_nbr + 7) // 8 * 8 if local and windowed else 0
    rows16 = torch.empty((N, stride16), dtype=torch.int16, device=dev) if stride16 else None
    ws = _ws(L.dmet_radius_workspace_bytes(N), dev) if windowed else None
    head = (x.data_ptr(), ptr.data_ptr(), B, N, D, float(r), max_nbr, 1 if skip_self else 0)
    fill, st = 1 if pad else 0, _stream(dev)
    out = (None if nbr is None else nbr.data_ptr(), cnt.data_ptr())
    rows = (None if rows16 is None else rows16.data_ptr(), stride16)
    if query is not None:
        name, args = "dmet_radius_xy_f32", (x.data_ptr(), ptr.data_ptr(), Nx, y.data_ptr(), ptr_y.data_ptr(), N, B, D,
                                            float(r), max_nbr, per_p, fill, *out, st)
    elif windowed:
        tail = (ws.data_ptr(), ws.numel(), st)
        if per is not None:
            name, args = "dmet_radius_windowed_periodic_f32", (*head, fill, per_p, *out, *rows, *tail)
        elif local:
            name, args = "dmet_radius_windowed_local_f32", (*head, fill, *out, *rows, *tail)
        else:
            name, args = "dmet_radius_windowed_f32", (*head, fill, *out, *tail)
    elif per is not None:
        name, args = "dmet_radius_periodic_f32", (*head, fill, per_p, *out, st)
    else:
        name, args = ("dmet_radius_f32" if pad else "dmet_radius_counted_f32"), (*head, *out, st)
    with _on(dev):
        _lib.check(getattr(L, name)(*args), name)
    return nbr, cnt, rows16


def radius_xy(x: torch.Tensor, ptr_x: torch.Tensor, y: torch.Tensor, ptr_y: torch.Tensor, r: float, max_nbr: int,
              period=None, pad: bool = True):
    """Two point sets (dmet_radius_xy_f32): for every row of y the first max_nbr rows of x (ascending id) of the same
    event within r.  (nbr[Ny,max_nbr] int32, cnt[Ny] int32); pad=False leaves the slots >= cnt[i] unwritten."""
    return _radius_build(x, ptr_x, r, max_nbr, False, pad, False, True, period, (y, ptr_y))[:2]


def radius(x: torch.Tensor, ptr: torch.Tensor, r: float, max_nbr: int, skip_self: bool = False,
           pad: bool = True, local: bool = False, int32_rows: bool = True, period=None):
    """(nbr[N,max_nbr] int32, cnt[N] int32).  pad=False leaves the slots >= cnt[i] unwritten instead of filling them
    with -1 (the fill is most of a 255-wide table's bytes); only for consumers that go by cnt.
    local=True: a third result, the rows again as event-local uint16 ids (int16-typed [N, roundup8(max_nbr)], slots
    cnt[i] .. roundup8(cnt[i]) - 1 = 0xFFFF, the rest unwritten) for gather_max_local_j16; None when the all-pairs
    form is selected.  int32_rows=False (with local=True, pad=False, windowed form): the int32 table is not written at all
    and comes back as None -- for callers whose consumers read the uint16 rows (graph.NeighborTable expands them on demand).
    period: None, or D floats, period[c] > 0 the circumference of coordinate c, 0 a plain coordinate
    (dmet_radius_periodic_f32 / dmet_radius_windowed_periodic_f32).  The window runs on coordinate 0, so period[0] > 0
    takes the all-pairs form (rows16 = None, as RADIUS_FORM == "sweep" does)."""
    out = _radius_build(x, ptr, r, max_nbr, skip_self, pad, local, int32_rows, period)
    return out if local else out[:2]


def radius_periodic(x: torch.Tensor, ptr: torch.Tensor, r: float, max_nbr: int, period, skip_self: bool = False,
                    pad: bool = True, local: bool = False, int32_rows: bool = True):
    """radius(..., period=period)."""
    return radius(x, ptr, r, max_nbr, skip_self, pad, local, int32_rows, period)


# ---- K2+K3 fused -----------------------------------------------------------------------------------------------
def node_linear_split(x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor],
                      sliced: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(P, Q) = (x (W1-W2)^T + b, x W2^T) as [N, Hout] tensors; sliced=True: the same values stored slice-major,
    [Hout/8][N][8], for gather_max(..., sliced=True) only (the returned tensors then have shape [Hout/8, N, 8])."""
    dev = _require_device(x, W, b)
    L = _lib.load()
    x = _f32a(x, "x"); W = _f32c(W, "W")
    N, Hin = x.shape
    Hout = W.shape[0]
    if W.shape[1] != 2 * Hin:
        raise ValueError(f"W must be [Hout, 2*Hin] = [*, {2 * Hin}], got {tuple(W.shape)}")
    if sliced and Hout % 8 != 0:
        raise ValueError("node_linear_split: sliced tables need Hout % 8 == 0")
    PQ = torch.empty((2, Hout // 8, N, 8) if sliced else (2, N, Hout), dtype=torch.float32, device=dev)
    bp = _f32c(b, "b").data_ptr() if b is not None else None
    _t = timer.record('node_linear_split', dev)
    with _on(dev):
        fn = L.dmet_node_linear_split_sliced_f32 if sliced else L.dmet_node_linear_split_f32
        _lib.check(fn(x.data_ptr(), N, Hin, Hout, W.data_ptr(), bp, PQ[0].data_ptr(), PQ[1].data_ptr(), _stream(dev)),
                   "dmet_node_linear_split_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return PQ[0], PQ[1]


def bn_node_linear_split(raw: torch.Tensor, residual: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                         mean: torch.Tensor, invstd: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor],
                         sliced: bool = False):
    """(y, P, Q): y = residual + BatchNorm(raw) (statistics given; the bits of bn_fwd's transform) and the dense layer
    node_linear_split(y, W, b, sliced) in ONE launch (dmet_bn_node_linear_split_f32), or None when the operands do not
    qualify (32 -> 32 features, 16-byte aligned vectors)."""
    dev = _require_device(raw, gamma, beta, mean, invstd, W)
    L = _lib.load()
    if raw.dim() != 2 or raw.shape[1] != 32 or tuple(W.shape) != (32, 64) or raw.dtype != torch.float32:
        return None
    raw, residual, vec, aligned = _bn_affine_operands("bn_node_linear_split", raw, residual, gamma, beta, mean, invstd)
    W = _f32c(W, "W")
    b = _f32c(b, "b") if b is not None else None
    if not aligned:
        return None
    N = raw.shape[0]
    y = torch.empty_like(raw)
    P, Q, layout, _ = _pq_tables(N, bool(sliced), dev)
    if N == 0:
        return y, P, Q
    _t = timer.record('node_linear_split', dev)
    with _on(dev):
        _lib.check(L.dmet_bn_node_linear_split_f32(raw.data_ptr(), _ptr(residual), *[v.data_ptr() for v in vec], y.data_ptr(),
                                                   N, 32, W.data_ptr(), _ptr(b), layout, P.data_ptr(), Q.data_ptr(),
                                                   _stream(dev)), "dmet_bn_node_linear_split_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return y, P, Q


def _gather_run(dev: torch.device, key: str, note: Optional[str], entry: str, *args) -> None:
    """One gather / scatter entry of the C ABI on dev's current stream (appended to args), inside a `key` bracket of the
    timer; `note`, if given, becomes last_gather_kernel.  A failure is reported under the name of the entry called."""
    _t = timer.record(key, dev)
    if note is not None:
        _note_gather(note)
    with _on(dev):
        _lib.check(getattr(_lib.load(), entry)(*args, _stream(dev)), entry)
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))


def _pq_shape(P: torch.Tensor, sliced: bool) -> Tuple[int, int]:
    """(N, H) of a row-major [N, H] table or of a slice-major [H/8, N, 8] one (node_linear_split(..., sliced=True))."""
    return (P.shape[1], P.shape[0] * 8) if sliced else (P.shape[0], P.shape[1])


def _check_nbr_local(nbr_local: Optional[torch.Tensor], nbr: torch.Tensor) -> None:
    if nbr_local is not None and (nbr_local.shape != nbr.shape or nbr_local.dtype != torch.int16
                                  or not nbr_local.is_contiguous()):
        raise ValueError("nbr_local must be the contiguous int16 [N, k] table of knn_local()")


def gather_max(P: torch.Tensor, Q: torch.Tensor, nbr: torch.Tensor, ptr: Optional[torch.Tensor],
               want_arg: bool, cnt: Optional[torch.Tensor] = None, lds: bool = False,
               nbr_local: Optional[torch.Tensor] = None, sliced: bool = False, mixed: bool = False,
               max_nodes: Optional[int] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """out = P + max over the rows of Q listed in nbr (+ uint8 arg).  lds=True: the caller knows every event fits
    the LDS image (<= 5119 nodes, k in LDS_GATHER_K, H % 8 == 0) -> LDS-resident kernel; mixed=True: some events do not,
    the form is chosen per event inside the call (row-major P / Q); else gathers come from L2.  max_nodes: the batch's
    largest event when the caller knows it (a hint: batches of small events run two 512-thread workgroups per CU)."""
    dev = _require_device(P, Q, nbr)
    N, H = _pq_shape(P, sliced)
    k = nbr.shape[1]
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    arg = torch.empty((N, H), dtype=torch.uint8, device=dev) if want_arg else None
    table = (P.data_ptr(), Q.data_ptr(), nbr.data_ptr())
    local = _ptr(nbr_local)
    events = (ptr.data_ptr(), ptr.numel() - 1) if ptr is not None else (None, 0)
    outs = (out.data_ptr(), arg.data_ptr() if want_arg else None)
    tail = (N, k, H) + outs
    lds_form = ptr is not None and H % 8 == 0 and GATHER_MAX_FORM != "l2-only"
    # the route: (entry, its arguments, what bench.py prints as the kernel)
    if mixed and cnt is None and not sliced and ptr is not None and GATHER_MAX_FORM == "auto":
        _check_nbr_local(nbr_local, nbr)
        entry, args = "dmet_gather_max_mixed_f32", table + (local,) + events + tail
        note = ("gather_max_lds_kernel (events <= 5119 nodes: Q slice resident in LDS) + gather_max_mlp_kernel "
                "(larger events: row gathers from L2), chosen per event in one call; row-major P/Q")
    elif sliced and cnt is None:      # [H/8, N, 8] tables of node_linear_split(..., sliced=True)
        if ptr is None or k not in LDS_GATHER_K or GATHER_MAX_FORM == "l2-only":
            raise ValueError("gather_max: slice-major tables are only read by the LDS-resident kernels")
        entry, args = "dmet_gather_max_lds_sliced_cap_f32", table + (local,) + events + tail + (int(max_nodes or 0),)
        note = ("gather_max_lds_kernel (per-event Q slice resident in LDS; slice-major P/Q, "
                + ("uint16 event-local ids)" if nbr_local is not None else "int32 ids)"))
    elif cnt is not None and lds and lds_form:
        entry = "dmet_gather_max_counted_lds_f32"
        args = table + (cnt.data_ptr(),) + events + (N, k, H, 1 if sliced else 0) + outs
        note = ("gather_max_lds_kernel, counted rows (radius table; Q slice resident in LDS"
                + (", slice-major P/Q)" if sliced else ")"))
    elif sliced:
        raise ValueError("gather_max: slice-major tables are only read by the LDS-resident kernels")
    elif cnt is not None:
        entry, args = "dmet_gather_max_counted_f32", table + (cnt.data_ptr(),) + tail
        note = "gather_max_kernel, counted rows (radius table; gathers from L2)"
    elif (lds or GATHER_MAX_FORM == "lds") and lds_form and nbr_local is not None and k in LDS_GATHER_K:
        _check_nbr_local(nbr_local, nbr)
        entry, args = "dmet_gather_max_lds16_f32", table + (local,) + events + tail
        note = "gather_max_lds_kernel (per-event Q slice resident in LDS; row-major P/Q, uint16 ids)"
    elif (lds or GATHER_MAX_FORM == "lds") and lds_form:
        entry, args = "dmet_gather_max_lds_f32", table + events + tail
        note = "gather_max_lds_kernel (per-event Q slice resident in LDS; row-major P/Q, int32 ids)"
    else:
        entry, args = "dmet_gather_max_f32", table + events + tail
        note = "gather_max_mlp_kernel (row gathers from L2; events too large for the LDS image)"
    _gather_run(dev, 'gather_max', note, entry, *args)
    return out, arg


def table_order_by_count(cnt: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """order[N] int32: per event, its local node indices grouped by slot count (deepest rows first)."""
    dev = _require_device(cnt, ptr)
    L = _lib.load()
    N = cnt.numel()
    order = torch.empty((N,), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_table_order_by_count(cnt.data_ptr(), ptr.data_ptr(), ptr.numel() - 1, N, order.data_ptr(),
                                               _stream(dev)), "dmet_table_order_by_count")
    return order


def gather_max_counted_j16(P: torch.Tensor, Q: torch.Tensor, nbr: torch.Tensor, cnt: torch.Tensor,
                           order: Optional[torch.Tensor], ptr: torch.Tensor, sliced: bool):
    """(out[N,H], argj[N,H] int16-typed uint16 winner ids) of the counted LDS gather (radius tables)."""
    dev = _require_device(P, Q, nbr, cnt, ptr)
    N, H = _pq_shape(P, sliced)
    k = nbr.shape[1]
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    argj = torch.empty((N, H), dtype=torch.int16, device=dev)
    _gather_run(dev, 'gather_max', "gather_max_lds_kernel, counted rows (radius table; Q slice resident in LDS, winner ids, "
                "rows ordered by depth" + (", slice-major P/Q)" if sliced else ")"), "dmet_gather_max_counted_lds_j16_f32",
                P.data_ptr(), Q.data_ptr(), nbr.data_ptr(), cnt.data_ptr(), _ptr(order),
                ptr.data_ptr(), ptr.numel() - 1, N, k, H, 1 if sliced else 0, out.data_ptr(), argj.data_ptr())
    return out, argj


def gather_max_local_j16(P: torch.Tensor, Q: torch.Tensor, rows16: torch.Tensor, cnt: torch.Tensor,
                         order: Optional[torch.Tensor], ptr: torch.Tensor, kmax: int, sliced: bool, want_arg: bool = True):
    """gather_max_counted_j16 reading the ids from the uint16 rows of radius(..., local=True): identical (out, argj);
    want_arg=False (inference): (out, None)."""
    dev = _require_device(P, Q, rows16, cnt, ptr)
    N, H = _pq_shape(P, sliced)
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    argj = torch.empty((N, H), dtype=torch.int16, device=dev) if want_arg else None
    _gather_run(dev, 'gather_max', "gather_max_lds_kernel, counted rows (radius table as event-local uint16 rows; Q slice "
                "resident in LDS, winner ids, rows ordered by depth" + (", slice-major P/Q)" if sliced else ")"),
                "dmet_gather_max_local_j16_f32", P.data_ptr(), Q.data_ptr(), rows16.data_ptr(), rows16.shape[1],
                cnt.data_ptr(), _ptr(order), ptr.data_ptr(), ptr.numel() - 1, N, kmax, H,
                1 if sliced else 0, out.data_ptr(), _ptr(argj))
    return out, argj


def gather_max_bwd_j16(g_out: torch.Tensor, argj: torch.Tensor, ptr: torch.Tensor,
                       max_nodes: Optional[int] = None, sliced: bool = False) -> torch.Tensor:
    """max_nodes: the batch's largest event when the caller knows it (a hint: workgroups sized for small events).
    sliced: gQ comes back slice-major, [8, N, 4] (for edgeconv_linear_bwd(..., gq_sliced=True): a scatter workgroup then
    writes one contiguous run instead of 16-byte pieces of 128-byte rows)."""
    dev = _require_device(g_out, argj, ptr)
    g_out = _f32a(g_out, "g_out")
    N, H = g_out.shape
    if argj.dtype != torch.int16 or argj.shape != g_out.shape or not argj.is_contiguous():
        raise TypeError("gather_max_bwd_j16: argj must be the contiguous int16 [N,H] tensor of gather_max_counted_j16")
    sliced = bool(sliced and H == 32)
    gQ = torch.empty((8, N, 4) if sliced else (N, H), dtype=torch.float32, device=dev)
    _gather_run(dev, 'gather_max_bwd', None, "dmet_gather_max_bwd_j16_sliced_f32" if sliced else "dmet_gather_max_bwd_j16_cap_f32",
                g_out.data_ptr(), argj.data_ptr(), ptr.data_ptr(), ptr.numel() - 1, N, H, gQ.data_ptr(), int(max_nodes or 0))
    return gQ


def edgeconv_fused_lds(x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor], nbr: torch.Tensor,
                       ptr: torch.Tensor, want_arg: bool):
    """EdgeConv(Linear(64->32), max) in one launch (LDS-resident Q slice per event); see include/dmet.h."""
    dev = _require_device(x, W, b, nbr, ptr)
    L = _lib.load()
    x = _f32a(x, "x"); W = _f32c(W, "W")
    N, Hin = x.shape
    Hout = W.shape[0]
    k = nbr.shape[1]
    out = torch.empty((N, Hout), dtype=torch.float32, device=dev)
    arg = torch.empty((N, Hout), dtype=torch.uint8, device=dev) if want_arg else None
    bp = _f32c(b, "b").data_ptr() if b is not None else None
    _t = timer.record('edgeconv_fused', dev)
    _note_gather("edgeconv_fused_lds_kernel (gather + edge-MLP + max in one launch)")
    with _on(dev):
        _lib.check(L.dmet_edgeconv_fused_lds_f32(x.data_ptr(), nbr.data_ptr(), ptr.data_ptr(), ptr.numel() - 1, N, k,
                                                 Hin, Hout, W.data_ptr(), bp, out.data_ptr(),
                                                 arg.data_ptr() if want_arg else None, _stream(dev)),
                   "dmet_edgeconv_fused_lds_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, arg


def edge_mlp2_supported(Hin: int, H1: int, H2: int, k: int) -> bool:
    return bool(_lib.load().dmet_edge_mlp2_supported(int(Hin), int(H1), int(H2), int(k)))


def edge_mlp2_bf16(x: torch.Tensor, nbr: torch.Tensor, W1: torch.Tensor, b1: Optional[torch.Tensor], W2: torch.Tensor,
                   b2: Optional[torch.Tensor], act2: bool, add: bool) -> torch.Tensor:
    """out[N,H2] = aggr_s nn([x_i || x_j - x_i]) for nn = Linear - ELU - Linear [- ELU] on the bf16 matrix cores,
    fused with the max / add aggregation over the fixed-width table (include/dmet.h: dmet_edge_mlp2_bf16)."""
    dev = _require_device(x, nbr, W1, W2, b1, b2)
    L = _lib.load()
    x = _f32a(x, "x"); W1 = _f32c(W1, "W1"); W2 = _f32c(W2, "W2")
    N, Hin = x.shape
    H1, H2, k = W1.shape[0], W2.shape[0], nbr.shape[1]
    if W1.shape[1] != 2 * Hin or W2.shape[1] != H1:
        raise ValueError(f"edge_mlp2: W1 must be [H1, {2 * Hin}] and W2 [H2, H1], got {tuple(W1.shape)}, {tuple(W2.shape)}")
    if nbr.dtype != torch.int32 or not nbr.is_contiguous():
        raise TypeError("edge_mlp2: nbr must be a contiguous int32 [N, k] table")
    out = torch.empty((N, H2), dtype=torch.float32, device=dev)
    _t = timer.record('edge_mlp2', dev)
    with _on(dev):
        _lib.check(L.dmet_edge_mlp2_bf16(x.data_ptr(), N, Hin, nbr.data_ptr(), k, W1.data_ptr(),
                                         _f32c(b1, "b1").data_ptr() if b1 is not None else None, H1, W2.data_ptr(),
                                         _f32c(b2, "b2").data_ptr() if b2 is not None else None, H2, 1 if act2 else 0,
                                         1 if add else 0, out.data_ptr(), _stream(dev)), "dmet_edge_mlp2_bf16")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out


def edge_mlp2_bn_bf16(x: torch.Tensor, nbr: torch.Tensor, W1: torch.Tensor, b1: Optional[torch.Tensor], W2: torch.Tensor,
                      b2: Optional[torch.Tensor], act2: bool, add: bool, gamma: Optional[torch.Tensor],
                      beta: Optional[torch.Tensor], eps: float, momentum: float, running_mean: Optional[torch.Tensor],
                      running_var: Optional[torch.Tensor], num_batches_tracked: Optional[torch.Tensor],
                      training: bool) -> torch.Tensor:
    """edge_mlp2_bf16 followed by BatchNorm1d(H2) over the edge messages, then the aggregation (include/dmet.h:
    dmet_edge_mlp2_bn_bf16); the running statistics are updated in place in training mode."""
    dev = _require_device(x, nbr, W1, W2, b1, b2, gamma, beta)
    L = _lib.load()
    x = _f32a(x, "x"); W1 = _f32c(W1, "W1"); W2 = _f32c(W2, "W2")
    N, Hin = x.shape
    H1, H2, k = W1.shape[0], W2.shape[0], nbr.shape[1]
    if W1.shape[1] != 2 * Hin or W2.shape[1] != H1:
        raise ValueError(f"edge_mlp2: W1 must be [H1, {2 * Hin}] and W2 [H2, H1], got {tuple(W1.shape)}, {tuple(W2.shape)}")
    if nbr.dtype != torch.int32 or not nbr.is_contiguous():
        raise TypeError("edge_mlp2: nbr must be a contiguous int32 [N, k] table")
    out = torch.empty((N, H2), dtype=torch.float32, device=dev)
    ptr = lambda t: _f32c(t, "param").data_ptr() if t is not None else None
    _t = timer.record('edge_mlp2', dev)
    with _on(dev):
        ws = _ws(L.dmet_edge_mlp2_bn_workspace_bytes(N, H2), dev)
        _lib.check(L.dmet_edge_mlp2_bn_bf16(x.data_ptr(), N, Hin, nbr.data_ptr(), k, W1.data_ptr(), ptr(b1), H1, W2.data_ptr(),
                                            ptr(b2), H2, 1 if act2 else 0, 1 if add else 0, ptr(gamma), ptr(beta), float(eps),
                                            float(momentum), ptr(running_mean), ptr(running_var),
                                            _ptr(num_batches_tracked), 1 if training else 0, out.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _stream(dev)),
                   "dmet_edge_mlp2_bn_bf16")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out


_EMLP_AGGR = {"max": 0, "add": 1, "sum": 1, "mean": 2}
# per-edge operand type of the three fused edge-MLP routes over a grouped edge list, for the docstrings
_EMLP_OPERANDS = {"f32": "fp32", "bf16": "bf16 matrix cores", "f16": "fp16 matrix cores (RNE, overflow to inf)"}


def _edge_arrays(rowptr, src, tgt, N, route="f32"):
    for name, t in (("rowptr", rowptr), ("src", src), ("tgt", tgt)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise TypeError(f"edge_mlp_{route}: {name} must be a contiguous int32 tensor")
    if rowptr.numel() != N + 1:
        raise ValueError(f"edge_mlp_{route}: rowptr must hold N + 1 = {N + 1} entries, got {rowptr.numel()}")
    if src.numel() != tgt.numel():
        raise ValueError(f"edge_mlp_{route}: src and tgt differ in length")
    return src.numel()


def _edge_mlp_supported(route, Hin: int, H1: int, H2: int) -> bool:
    """The widths dmet_edge_mlp_{route}_supported takes (include/dmet.h)."""
    return bool(getattr(_lib.load(), f"dmet_edge_mlp_{route}_supported")(int(Hin), int(H1), int(H2)))


def _edge_mlp_fwd(route, x: torch.Tensor, rowptr: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor, W1: torch.Tensor,
                  b1: Optional[torch.Tensor], W2: torch.Tensor, b2: Optional[torch.Tensor], act2: bool, aggr: str,
                  bn: int = 0, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                  eps: float = 1e-5, momentum: float = 0.1, running_mean: Optional[torch.Tensor] = None,
                  running_var: Optional[torch.Tensor] = None, num_batches_tracked: Optional[torch.Tensor] = None):
    """out[N, H2] = aggr_e nn([x_tgt || x_src - x_tgt]) over a grouped edge list, nn = Linear - ELU - Linear [- ELU]
    [- BatchNorm1d] (include/dmet.h: dmet_edge_mlp_fwd_{route}; per-edge products: {operands}).  fp32 inputs, parameters
    and output; a 16-bit route rounds h1 and W2 inside the kernel only.  Returns (out, state); `state` is what
    edge_mlp_bwd_{route} needs (pq, agg, win, bnstat).  bn: 0 none, 1 training (statistics moved in place), 2 eval."""
    dev = _require_device(x, rowptr, src, tgt, W1, W2, b1, b2, gamma, beta)
    L = _lib.load()
    x = _f32c(x, "x"); W1 = _f32c(W1, "W1"); W2 = _f32c(W2, "W2")
    N, Hin = x.shape
    H1, H2 = W1.shape[0], W2.shape[0]
    if W1.shape[1] != 2 * Hin or W2.shape[1] != H1:
        raise ValueError(f"edge_mlp_{route}: W1 must be [H1, {2 * Hin}] and W2 [H2, H1], got {tuple(W1.shape)}, {tuple(W2.shape)}")
    if aggr not in _EMLP_AGGR:
        raise ValueError(f"edge_mlp_{route}: unsupported aggr {aggr!r}")
    E = _edge_arrays(rowptr, src, tgt, N, route)
    out = torch.empty((N, H2), dtype=torch.float32, device=dev)
    pq = torch.empty((N, 2 * H1), dtype=torch.float32, device=dev)
    agg = torch.empty((2 if aggr == "max" and bn else 1, N, H2), dtype=torch.float32, device=dev)
    win = torch.empty((2 if bn else 1, N, H2), dtype=torch.int32, device=dev) if aggr == "max" else None
    bnstat = torch.empty((4, H2), dtype=torch.float32, device=dev)
    p = lambda t: _f32c(t, "param").data_ptr() if t is not None else None
    _t = timer.record(f'edge_mlp_{route}', dev)
    with _on(dev):
        ws = _ws(getattr(L, f"dmet_edge_mlp_{route}_workspace_bytes")(N, E, Hin, H1, H2), dev)
        call = getattr(L, f"dmet_edge_mlp_fwd_{route}")
        _lib.check(call(x.data_ptr(), N, Hin, rowptr.data_ptr(), src.data_ptr(), tgt.data_ptr(), E,
                        W1.data_ptr(), p(b1), H1, W2.data_ptr(), p(b2), H2, 1 if act2 else 0,
                        _EMLP_AGGR[aggr], int(bn), p(gamma), p(beta), float(eps), float(momentum),
                        p(running_mean), p(running_var), _ptr(num_batches_tracked),
                        out.data_ptr(), pq.data_ptr(), agg.data_ptr(), _ptr(win), bnstat.data_ptr(), ws.data_ptr(),
                        ws.numel(), _stream(dev)), f"dmet_edge_mlp_fwd_{route}")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, (pq, agg, win, bnstat)


def _xty_wide(A: torch.Tensor, Bm: torch.Tensor) -> torch.Tensor:
    """A^T B for widths above dmet_xty_f32's 64 columns: 64 x 64 tiles, each one deterministic call."""
    Ha, Hb = A.shape[1], Bm.shape[1]
    if Ha <= 64 and Hb <= 64:
        return xty(A, Bm)
    rows = []
    for a0 in range(0, Ha, 64):
        Ac = A[:, a0:a0 + 64].contiguous()
        rows.append(torch.cat([xty(Ac, Bm[:, b0:b0 + 64].contiguous()) for b0 in range(0, Hb, 64)], dim=1))
    return torch.cat(rows, dim=0)


def _edge_mlp_bwd(route, g_out: torch.Tensor, x: torch.Tensor, rowptr: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor,
                  srcptr: torch.Tensor, srcperm: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                  b2: Optional[torch.Tensor], act2: bool, aggr: str, bn: int, state, want_x: bool = True,
                  want_w1: bool = True, want_b1: bool = True):
    """Gradients of edge_mlp_fwd_{route} (include/dmet.h: dmet_edge_mlp_bwd_{route}; per-edge products g_h1 and gW2:
    {operands}, everything else fp32): (gx, gW1, gb1, gW2, gb2, ggamma, gbeta); gx / gW1 / gb1 are None when not wanted,
    ggamma / gbeta when bn == 0."""
    dev = _require_device(g_out, x, rowptr, src, tgt, srcptr, srcperm, W1, W2, b2)
    L = _lib.load()
    x = _f32c(x, "x"); W1 = _f32c(W1, "W1"); W2 = _f32c(W2, "W2"); g_out = _f32c(g_out, "g_out")
    N, Hin = x.shape
    H1, H2 = W1.shape[0], W2.shape[0]
    E = _edge_arrays(rowptr, src, tgt, N, route)
    if srcptr.dtype != torch.int32 or srcperm.dtype != torch.int32 or srcptr.numel() != N + 1:
        raise TypeError(f"edge_mlp_{route}: srcptr [N + 1] and srcperm must be int32 (EdgeList.by_source())")
    if tuple(g_out.shape) != (N, H2):
        raise ValueError(f"edge_mlp_{route}: g_out must be [{N}, {H2}], got {tuple(g_out.shape)}")
    pq, agg, win, bnstat = state
    gx = torch.empty((N, Hin), dtype=torch.float32, device=dev) if want_x else None
    gpq = torch.empty((N, 2 * H1), dtype=torch.float32, device=dev)
    gW2 = torch.empty((H2, H1), dtype=torch.float32, device=dev)
    gb2 = torch.empty((H2,), dtype=torch.float32, device=dev)
    ggamma = torch.empty((H2,), dtype=torch.float32, device=dev) if bn else None
    gbeta = torch.empty((H2,), dtype=torch.float32, device=dev) if bn else None
    _t = timer.record(f'edge_mlp_{route}_bwd', dev)
    with _on(dev):
        ws = _ws(getattr(L, f"dmet_edge_mlp_{route}_workspace_bytes")(N, E, Hin, H1, H2), dev)
        call = getattr(L, f"dmet_edge_mlp_bwd_{route}")
        _lib.check(call(x.data_ptr(), N, Hin, rowptr.data_ptr(), src.data_ptr(), tgt.data_ptr(), E,
                        srcptr.data_ptr(), srcperm.data_ptr(), W1.data_ptr(), H1, W2.data_ptr(),
                        _ptr(_f32c(b2, "b2") if b2 is not None else None), H2, 1 if act2 else 0,
                        _EMLP_AGGR[aggr], int(bn), pq.data_ptr(), agg.data_ptr(), _ptr(win),
                        bnstat.data_ptr(), g_out.data_ptr(), _ptr(gx), gpq.data_ptr(), gW2.data_ptr(),
                        gb2.data_ptr(), _ptr(ggamma), _ptr(gbeta), ws.data_ptr(), ws.numel(), _stream(dev)),
                   f"dmet_edge_mlp_bwd_{route}")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    gW1 = gb1 = None
    gP = gpq[:, :H1]
    if want_w1:
        if N == 0:
            gW1 = torch.zeros_like(W1)
        else:
            # a node without in- or out-edges has gP = gQ = 0: its x row is dropped from the product, so that a node no
            # edge reads (a non-finite kNN query) adds nothing instead of 0 * NaN (exact for finite x)
            isolated = (rowptr[1:] == rowptr[:-1]) & (srcptr[1:] == srcptr[:-1])
            C = _xty_wide(gpq, x.masked_fill(isolated.view(-1, 1), 0.0))   # [2 H1, Hin] = [gP^T x ; gQ^T x]
            gW1 = torch.cat([C[:H1], C[H1:] - C[:H1]], dim=1)
    if want_b1:
        gb1 = xty_wide_ones(gP) if N else torch.zeros((H1,), dtype=torch.float32, device=dev)
    return gx, gW1, gb1, gW2, gb2, ggamma, gbeta


def _bind_route(impl, name: str, route: str):
    """`impl` with its route fixed, under the public name: a module attribute of its own, so that a test can patch it."""
    def bound(*args, **kwargs):
        return impl(route, *args, **kwargs)
    bound.__name__ = bound.__qualname__ = name
    sig = inspect.signature(impl)
    bound.__signature__ = sig.replace(parameters=list(sig.parameters.values())[1:])     # impl's, without `route`
    bound.__doc__ = impl.__doc__.replace("{route}", route).replace("{operands}", _EMLP_OPERANDS[route])
    return bound


edge_mlp_f32_supported = _bind_route(_edge_mlp_supported, "edge_mlp_f32_supported", "f32")
edge_mlp_bf16_supported = _bind_route(_edge_mlp_supported, "edge_mlp_bf16_supported", "bf16")
edge_mlp_f16_supported = _bind_route(_edge_mlp_supported, "edge_mlp_f16_supported", "f16")
edge_mlp_fwd_f32 = _bind_route(_edge_mlp_fwd, "edge_mlp_fwd_f32", "f32")
edge_mlp_fwd_bf16 = _bind_route(_edge_mlp_fwd, "edge_mlp_fwd_bf16", "bf16")
edge_mlp_fwd_f16 = _bind_route(_edge_mlp_fwd, "edge_mlp_fwd_f16", "f16")
edge_mlp_bwd_f32 = _bind_route(_edge_mlp_bwd, "edge_mlp_bwd_f32", "f32")
edge_mlp_bwd_bf16 = _bind_route(_edge_mlp_bwd, "edge_mlp_bwd_bf16", "bf16")
edge_mlp_bwd_f16 = _bind_route(_edge_mlp_bwd, "edge_mlp_bwd_f16", "f16")


def xty_wide_ones(A: torch.Tensor) -> torch.Tensor:
    """Column sums of A[N, H] through dmet_xty_f32 (fixed order, deterministic)."""
    ones = torch.ones((A.shape[0], 1), dtype=torch.float32, device=A.device)
    return _xty_wide(ones, A).reshape(-1)


def node_linear_split_bf16(x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16-MFMA variant: P fp32 [N,H], Q as bf16 [N,H] (gathered table)."""
    dev = _require_device(x, W, b)
    L = _lib.load()
    x = _f32a(x, "x"); W = _f32c(W, "W")
    N, Hin = x.shape
    Hout = W.shape[0]
    P = torch.empty((N, Hout), dtype=torch.float32, device=dev)
    Qh = torch.empty((N, Hout), dtype=torch.bfloat16, device=dev)
    bp = _f32c(b, "b").data_ptr() if b is not None else None
    _t = timer.record('node_linear_split', dev)
    with _on(dev):
        _lib.check(L.dmet_node_linear_split_bf16(x.data_ptr(), N, Hin, Hout, W.data_ptr(), bp, P.data_ptr(),
                                                 Qh.data_ptr(), _stream(dev)), "dmet_node_linear_split_bf16")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return P, Qh


def gather_max_bf16q(P: torch.Tensor, Qh: torch.Tensor, nbr: torch.Tensor, want_arg: bool):
    dev = _require_device(P, Qh, nbr)
    L = _lib.load()
    N, H = P.shape
    k = nbr.shape[1]
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    arg = torch.empty((N, H), dtype=torch.uint8, device=dev) if want_arg else None
    _t = timer.record('gather_max', dev)
    _note_gather("gather_max_bf16q_kernel (gather + max over the bf16 Q table, gathers from L2)")
    with _on(dev):
        _lib.check(L.dmet_gather_max_bf16q(P.data_ptr(), Qh.data_ptr(), nbr.data_ptr(), N, k, H, out.data_ptr(),
                                           arg.data_ptr() if want_arg else None, _stream(dev)), "dmet_gather_max_bf16q")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, arg


def gather_max_bwd(g_out: torch.Tensor, arg: torch.Tensor, rev_ptr: torch.Tensor, rev_slot: torch.Tensor,
                   k: int) -> torch.Tensor:
    dev = _require_device(g_out, arg, rev_ptr, rev_slot)
    L = _lib.load()
    g_out = _f32a(g_out, "g_out")
    N, H = g_out.shape
    gQ = torch.empty((N, H), dtype=torch.float32, device=dev)
    _t = timer.record('gather_max_bwd', dev)
    with _on(dev):
        _lib.check(L.dmet_gather_max_bwd_f32(g_out.data_ptr(), arg.data_ptr(), rev_ptr.data_ptr(),
                                             rev_slot.data_ptr(), N, k, H, gQ.data_ptr(), _stream(dev)),
                   "dmet_gather_max_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return gQ


def _i32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.int32:
        raise TypeError(f"{name} must be int32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def gather_sum_table(P: torch.Tensor, Q: torch.Tensor, nbr: torch.Tensor, cnt: Optional[torch.Tensor],
                     mean: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out[N,H], deg[N] int32): out = deg P + sum of the Q rows listed in nbr (mean: P + that sum / deg), 0 for a row
    without neighbours.  cnt (radius tables): only the first cnt[i] slots of row i."""
    dev = _require_device(P, Q, nbr, cnt)
    L = _lib.load()
    P = _f32c(P, "P"); Q = _f32c(Q, "Q"); nbr = _i32c(nbr, "nbr")
    N, H = P.shape
    k = nbr.shape[1]
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    deg = torch.empty((N,), dtype=torch.int32, device=dev)
    cp = _i32c(cnt, "cnt").data_ptr() if cnt is not None else None
    _t = timer.record('gather_sum', dev)
    with _on(dev):
        _lib.check(L.dmet_gather_sum_table_f32(P.data_ptr(), Q.data_ptr(), nbr.data_ptr(), cp, N, k, H, int(mean),
                                               out.data_ptr(), deg.data_ptr(), _stream(dev)),
                   "dmet_gather_sum_table_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, deg


def gather_sum_csr(P: torch.Tensor, Q: torch.Tensor, rowptr: torch.Tensor, src: torch.Tensor,
                   mean: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """gather_sum_table over a by-target edge list (rowptr[N+1], src[E] int32)."""
    dev = _require_device(P, Q, rowptr, src)
    L = _lib.load()
    P = _f32c(P, "P"); Q = _f32c(Q, "Q"); rowptr = _i32c(rowptr, "rowptr"); src = _i32c(src, "src")
    N, H = P.shape
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    deg = torch.empty((N,), dtype=torch.int32, device=dev)
    _t = timer.record('gather_sum', dev)
    with _on(dev):
        _lib.check(L.dmet_gather_sum_csr_f32(P.data_ptr(), Q.data_ptr(), rowptr.data_ptr(), src.data_ptr(), N, H,
                                             int(mean), out.data_ptr(), deg.data_ptr(), _stream(dev)),
                   "dmet_gather_sum_csr_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, deg


def gather_sum_bwd(g_out: torch.Tensor, deg: torch.Tensor, rev_ptr: torch.Tensor, rev_idx: torch.Tensor,
                   tgt: Optional[torch.Tensor], k: int, mean: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(gP, gQ) of gather_sum_table / gather_sum_csr.  Tables: tgt None, k the table width and (rev_ptr, rev_idx) =
    NeighborTable.reverse(); edge lists: (rev_ptr, rev_idx) = EdgeList.by_source() and tgt = EdgeList.tgt (k ignored)."""
    dev = _require_device(g_out, deg, rev_ptr, rev_idx, tgt)
    L = _lib.load()
    g_out = _f32a(g_out, "g_out"); deg = _i32c(deg, "deg")
    rev_ptr = _i32c(rev_ptr, "rev_ptr"); rev_idx = _i32c(rev_idx, "rev_idx")
    N, H = g_out.shape
    gPQ = torch.empty((2, N, H), dtype=torch.float32, device=dev)
    tp = _i32c(tgt, "tgt").data_ptr() if tgt is not None else None
    _t = timer.record('gather_sum_bwd', dev)
    with _on(dev):
        _lib.check(L.dmet_gather_sum_bwd_f32(g_out.data_ptr(), deg.data_ptr(), rev_ptr.data_ptr(), rev_idx.data_ptr(),
                                             tp, N, 0 if tgt is not None else k, H, int(mean), gPQ[0].data_ptr(),
                                             gPQ[1].data_ptr(), _stream(dev)),
                   "dmet_gather_sum_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return gPQ[0], gPQ[1]


GRAVNET_MAX_S = 16      # coordinates of the learned space (include/dmet.h, "GravNet aggregation")
GRAVNET_MAX_P = 128     # DMET_MAX_H
GRAVNET_MAX_K = 64      # DMET_MAX_K


def gravnet_check_shapes(h: torch.Tensor, s_src: torch.Tensor, s_tgt: torch.Tensor, nbr: torch.Tensor) -> None:
    """The argument errors of the GravNet entries, raised from shapes alone (before any device is asked for)."""
    if h.dim() != 2 or s_src.dim() != 2 or s_tgt.dim() != 2 or nbr.dim() != 2:
        raise ValueError(f"gravnet: h [Ns, P], s [N, S] and nbr [Nt, k] must be 2-D, got {tuple(h.shape)}, "
                         f"{tuple(s_src.shape)}, {tuple(s_tgt.shape)}, {tuple(nbr.shape)}")
    P, S, k = h.shape[1], s_src.shape[1], nbr.shape[1]
    if not 1 <= S <= GRAVNET_MAX_S:
        raise ValueError(f"gravnet: S={S} coordinates, supported 1..{GRAVNET_MAX_S}")
    if not 1 <= P <= GRAVNET_MAX_P:
        raise ValueError(f"gravnet: P={P} propagated features, supported 1..{GRAVNET_MAX_P}")
    if not 1 <= k <= GRAVNET_MAX_K:
        raise ValueError(f"gravnet: k={k}, supported 1..{GRAVNET_MAX_K}")
    if s_tgt.shape[1] != S:
        raise ValueError(f"gravnet: source coordinates have {S} columns, target coordinates {s_tgt.shape[1]}")
    if h.shape[0] != s_src.shape[0]:
        raise ValueError(f"gravnet: h has {h.shape[0]} rows, the source coordinates {s_src.shape[0]}")
    if nbr.shape[0] != s_tgt.shape[0]:
        raise ValueError(f"gravnet: the table has {nbr.shape[0]} rows, the target coordinates {s_tgt.shape[0]}")


def gravnet_fwd(h: torch.Tensor, s_src: torch.Tensor, s_tgt: torch.Tensor,
                nbr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(out[Nt, 2P] = [mean | max] of exp(-10 d) h_j over row i of nbr, arg[Nt, P] uint8, cnt[Nt] int32); see
    include/dmet.h, dmet_gravnet_fwd_f32.  The one-set form passes the same tensor as s_src and s_tgt."""
    gravnet_check_shapes(h, s_src, s_tgt, nbr)
    dev = _require_device(h, s_src, s_tgt, nbr)
    L = _lib.load()
    h = _f32c(h, "h"); s_src = _f32c(s_src, "s"); s_tgt = _f32c(s_tgt, "s_dst"); nbr = _i32c(nbr, "nbr")
    (Ns, P), S = h.shape, s_src.shape[1]
    Nt, k = nbr.shape
    out = torch.empty((Nt, 2 * P), dtype=torch.float32, device=dev)
    arg = torch.empty((Nt, P), dtype=torch.uint8, device=dev)
    cnt = torch.empty((Nt,), dtype=torch.int32, device=dev)
    _t = timer.record('gravnet_fwd', dev)
    with _on(dev):
        _lib.check(L.dmet_gravnet_fwd_f32(s_tgt.data_ptr(), s_src.data_ptr(), h.data_ptr(), nbr.data_ptr(), Nt, Ns, k, S, P,
                                          out.data_ptr(), arg.data_ptr(), cnt.data_ptr(), _stream(dev)),
                   "dmet_gravnet_fwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, arg, cnt


def gravnet_bwd(g_out: torch.Tensor, h: torch.Tensor, s_src: torch.Tensor, s_tgt: torch.Tensor, nbr: torch.Tensor,
                rev_ptr: torch.Tensor, rev_pos: torch.Tensor, arg: torch.Tensor,
                cnt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(g_h[Ns, P], g_s_src[Ns, S], g_s_tgt[Nt, S]) of gravnet_fwd; (rev_ptr, rev_pos) = the table's reverse index over
    the Ns sources.  See include/dmet.h, dmet_gravnet_bwd_f32."""
    gravnet_check_shapes(h, s_src, s_tgt, nbr)
    dev = _require_device(g_out, h, s_src, s_tgt, nbr, rev_ptr, rev_pos, arg, cnt)
    L = _lib.load()
    h = _f32c(h, "h"); s_src = _f32c(s_src, "s"); s_tgt = _f32c(s_tgt, "s_dst"); nbr = _i32c(nbr, "nbr")
    g_out = _f32c(g_out, "g_out")
    rev_ptr = _i32c(rev_ptr, "rev_ptr"); rev_pos = _i32c(rev_pos, "rev_pos"); cnt = _i32c(cnt, "cnt")
    (Ns, P), S = h.shape, s_src.shape[1]
    Nt, k = nbr.shape
    if g_out.shape != (Nt, 2 * P) or arg.shape != (Nt, P) or arg.dtype != torch.uint8 or not arg.is_contiguous():
        raise ValueError(f"gravnet_bwd: g_out must be [{Nt}, {2 * P}] and arg a contiguous uint8 [{Nt}, {P}]")
    if rev_ptr.numel() != Ns + 1 or rev_pos.numel() < Nt * k or cnt.numel() != Nt:
        raise ValueError(f"gravnet_bwd: reverse index / cnt do not fit a [{Nt}, {k}] table over {Ns} sources")
    g_h = torch.empty((Ns, P), dtype=torch.float32, device=dev)
    g_s_src = torch.empty((Ns, S), dtype=torch.float32, device=dev)
    g_s_tgt = torch.empty((Nt, S), dtype=torch.float32, device=dev)
    g_d = torch.empty((Nt, k), dtype=torch.float32, device=dev)      # the one per-edge buffer: 4 B per slot
    _t = timer.record('gravnet_bwd', dev)
    with _on(dev):
        _lib.check(L.dmet_gravnet_bwd_f32(s_tgt.data_ptr(), s_src.data_ptr(), h.data_ptr(), nbr.data_ptr(),
                                          rev_ptr.data_ptr(), rev_pos.data_ptr(), arg.data_ptr(), cnt.data_ptr(),
                                          g_out.data_ptr(), Nt, Ns, k, S, P, g_d.data_ptr(), g_s_tgt.data_ptr(),
                                          g_s_src.data_ptr(), g_h.data_ptr(), _stream(dev)), "dmet_gravnet_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return g_h, g_s_src, g_s_tgt


INTERPOLATE_MAX_F = 256           # features per row (include/dmet.h, "Interpolation")
INTERPOLATE_MAX_K = GRAVNET_MAX_K   # DMET_MAX_K


def _interpolate_limits(F: int, k: int) -> None:
    if not 1 <= F <= INTERPOLATE_MAX_F:
        raise ValueError(f"interpolate: F={F} features, supported 1..{INTERPOLATE_MAX_F}")
    if not 1 <= k <= INTERPOLATE_MAX_K:
        raise ValueError(f"interpolate: k={k}, supported 1..{INTERPOLATE_MAX_K}")


def interpolate_check_shapes(x: torch.Tensor, nbr: torch.Tensor, dist: torch.Tensor) -> None:
    """The argument errors of the interpolation entries, raised from shapes alone (before any device is asked for)."""
    if x.dim() != 2 or nbr.dim() != 2 or dist.dim() != 2:
        raise ValueError(f"interpolate: x [Ns, F], nbr [Nt, k] and dist [Nt, k] must be 2-D, got {tuple(x.shape)}, "
                         f"{tuple(nbr.shape)}, {tuple(dist.shape)}")
    _interpolate_limits(x.shape[1], nbr.shape[1])
    if tuple(dist.shape) != tuple(nbr.shape):
        raise ValueError(f"interpolate: the table is {tuple(nbr.shape)}, its distances {tuple(dist.shape)}")


def interpolate_fwd(x: torch.Tensor, nbr: torch.Tensor, dist: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out[Nt, F] = sum over row i of nbr of r_t x[j], r_t = w_t / W_i, w_t = 1 / clamp(dist[i,t], 1e-16); wsum[Nt] = W_i);
    see include/dmet.h, dmet_interpolate_fwd_f32.  The outputs are zero-filled allocations: the entry writes all of them."""
    interpolate_check_shapes(x, nbr, dist)
    dev = _require_device(x, nbr, dist)
    L = _lib.load()
    x = _f32c(x, "x"); nbr = _i32c(nbr, "nbr"); dist = _f32c(dist, "dist")
    (Ns, F), (Nt, k) = x.shape, nbr.shape
    out = torch.zeros((Nt, F), dtype=torch.float32, device=dev)
    wsum = torch.zeros((Nt,), dtype=torch.float32, device=dev)
    _t = timer.record('interpolate_fwd', dev)
    with _on(dev):
        _lib.check(L.dmet_interpolate_fwd_f32(_ptr(x), nbr.data_ptr(), dist.data_ptr(), Nt, Ns, k, F, out.data_ptr(),
                                              wsum.data_ptr(), _stream(dev)), "dmet_interpolate_fwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, wsum


def interpolate_bwd(g_out: torch.Tensor, dist: torch.Tensor, wsum: torch.Tensor, rev_ptr: torch.Tensor,
                    rev_pos: torch.Tensor, Ns: int) -> torch.Tensor:
    """g_x[Ns, F] of interpolate_fwd; (rev_ptr, rev_pos) = the table's reverse index over the Ns sources.  See
    include/dmet.h, dmet_interpolate_bwd_f32."""
    if g_out.dim() != 2 or dist.dim() != 2 or g_out.shape[0] != dist.shape[0]:
        raise ValueError(f"interpolate_bwd: g_out [Nt, F] and dist [Nt, k] must be 2-D over the same rows, got "
                         f"{tuple(g_out.shape)} and {tuple(dist.shape)}")
    (Nt, F), k, Ns = g_out.shape, dist.shape[1], int(Ns)
    _interpolate_limits(F, k)
    if Ns < 0 or wsum.numel() != Nt or rev_ptr.numel() != Ns + 1 or rev_pos.numel() < Nt * k:
        raise ValueError(f"interpolate_bwd: wsum / reverse index do not fit a [{Nt}, {k}] table over {Ns} sources")
    dev = _require_device(g_out, dist, wsum, rev_ptr, rev_pos)
    L = _lib.load()
    g_out = _f32c(g_out, "g_out"); dist = _f32c(dist, "dist"); wsum = _f32c(wsum, "wsum")
    rev_ptr = _i32c(rev_ptr, "rev_ptr"); rev_pos = _i32c(rev_pos, "rev_pos")
    g_x = torch.zeros((Ns, F), dtype=torch.float32, device=dev)
    _t = timer.record('interpolate_bwd', dev)
    with _on(dev):
        _lib.check(L.dmet_interpolate_bwd_f32(_ptr(g_out), _ptr(dist), _ptr(wsum), rev_ptr.data_ptr(), rev_pos.data_ptr(),
                                              Nt, Ns, k, F, _ptr(g_x), _stream(dev)), "dmet_interpolate_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return g_x


MULTI_AGGR_MAX_F = 256            # features per row (include/dmet.h, "Multi-aggregation")
MULTI_AGGR_MAX_K = GRAVNET_MAX_K    # DMET_MAX_K: the width of a table
MULTI_AGGR_KINDS = {"sum": 1, "mean": 2, "min": 3, "max": 4, "var": 5, "std": 6}     # the ABI's codes


def multi_aggr_code(aggrs) -> int:
    """The `aggrs` argument of the multi-aggregation entries: the requested statistics, four bits each from the lowest in
    request order.  Unknown names, an empty request and a name given twice are ValueErrors."""
    if isinstance(aggrs, str) or not aggrs:
        raise ValueError(f"multi_aggr: aggrs must be a non-empty list of {sorted(MULTI_AGGR_KINDS)}, got {aggrs!r}")
    names = list(aggrs)
    for a in names:
        if a not in MULTI_AGGR_KINDS:
            raise ValueError(f"multi_aggr: unknown aggregator {a!r}, supported {sorted(MULTI_AGGR_KINDS)}")
    if len(set(names)) != len(names):
        raise ValueError(f"multi_aggr: an aggregator may be requested once, got {names}")
    return sum(MULTI_AGGR_KINDS[a] << (4 * s) for s, a in enumerate(names))


def multi_aggr_check_shapes(x: torch.Tensor, aggrs, groups: int, num_targets: int, num_sources: int,
                            width: Optional[int] = None) -> None:
    """The argument errors of the multi-aggregation entries, raised from shapes alone (before any device is asked for).
    The graph has num_targets rows over num_sources sources; width: the table form's k (None: an edge list)."""
    multi_aggr_code(aggrs)
    if x.dim() != 2:
        raise ValueError(f"multi_aggr: x must be [Ns, F], got {tuple(x.shape)}")
    F = x.shape[1]
    if not 1 <= F <= MULTI_AGGR_MAX_F:
        raise ValueError(f"multi_aggr: F={F} features, supported 1..{MULTI_AGGR_MAX_F}")
    if not isinstance(groups, int) or isinstance(groups, bool) or groups < 1 or F % groups:
        raise ValueError(f"multi_aggr: groups={groups!r} must be a positive int that divides F={F}")
    if width is not None and not 1 <= width <= MULTI_AGGR_MAX_K:
        raise ValueError(f"multi_aggr: k={width}, supported 1..{MULTI_AGGR_MAX_K}")
    if x.shape[0] != num_sources:
        raise ValueError(f"multi_aggr: the graph indexes {num_sources} sources, x has {x.shape[0]} rows")
    if num_targets < 0:
        raise ValueError(f"multi_aggr: {num_targets} target rows")


def _multi_aggr_fwd(x: torch.Tensor, idx: torch.Tensor, rowptr: Optional[torch.Tensor], num_targets: int, aggrs,
                    groups: int = 1):
    """(out[Nt, G, A, F/G], count[Nt] int32, saved) of the requested statistics over a table (idx = nbr[Nt, k], rowptr
    None) or a grouped edge list (idx = src[E], rowptr[Nt+1]); saved = (mean, var, argmin, argmax), each [Nt, F] or None
    when the request does not need it.  See include/dmet.h, dmet_multi_aggr_fwd_f32.  Not public, like _gat_fwd: pna.py and
    scatter.py are the callers."""
    Nt = int(num_targets)
    multi_aggr_check_shapes(x, aggrs, groups, Nt, x.shape[0], idx.shape[1] if rowptr is None and idx.dim() == 2 else None)
    code = multi_aggr_code(aggrs)
    dev = _require_device(x, idx, rowptr)
    L = _lib.load()
    x = _f32c(x, "x")
    idx, rowptr, E, width, _M = _row_graph("multi_aggr", idx, rowptr, Nt)
    Ns, F = x.shape
    A = len(aggrs)
    second = "var" in aggrs or "std" in aggrs
    out = torch.empty((Nt, groups, A, F // groups), dtype=torch.float32, device=dev)
    count = torch.empty((Nt,), dtype=torch.int32, device=dev)
    stats = torch.empty((2, Nt, F), dtype=torch.float32, device=dev) if second else None
    args = torch.empty((2, Nt, F), dtype=torch.int32, device=dev) if ("min" in aggrs or "max" in aggrs) else None
    mean, var = (stats[0], stats[1]) if second else (None, None)
    amin = args[0] if "min" in aggrs else None
    amax = args[1] if "max" in aggrs else None
    _t = timer.record('multi_aggr_fwd', dev)
    with _on(dev):
        _lib.check(L.dmet_multi_aggr_fwd_f32(_ptr(x), _ptr(idx), None if rowptr is None else rowptr.data_ptr(), Nt, Ns, E,
                                             width, F, groups, code, _ptr(out), _ptr(count), _ptr(mean), _ptr(var),
                                             _ptr(amin), _ptr(amax), _stream(dev)), "dmet_multi_aggr_fwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, count, (mean, var, amin, amax)


def _multi_aggr_bwd(g_out: torch.Tensor, x: torch.Tensor, count: torch.Tensor, saved, rev_ptr: torch.Tensor,
                    rev_pos: torch.Tensor, tgt: Optional[torch.Tensor], width: Optional[int], aggrs,
                    groups: int = 1) -> torch.Tensor:
    """g_x[Ns, F] of _multi_aggr_fwd; (rev_ptr, rev_pos) = the graph's by-source index, width = the table's k or None for
    a list, whose tgt[E] names the row of every position.  See include/dmet.h, dmet_multi_aggr_bwd_f32."""
    Nt = int(count.numel())
    multi_aggr_check_shapes(x, aggrs, groups, Nt, x.shape[0], width)
    code = multi_aggr_code(aggrs)
    Ns, F = x.shape
    A = len(aggrs)
    mean, var, amin, amax = saved
    if tuple(g_out.shape) != (Nt, groups, A, F // groups):
        raise ValueError(f"multi_aggr_bwd: g_out must be [{Nt}, {groups}, {A}, {F // groups}], got {tuple(g_out.shape)}")
    dev = _require_device(g_out, x, count, mean, var, amin, amax, rev_ptr, rev_pos, tgt)
    L = _lib.load()
    x = _f32c(x, "x"); g_out = _f32c(g_out, "g_out")
    rev_ptr = _i32c(rev_ptr, "rev_ptr"); rev_pos = _i32c(rev_pos, "rev_pos")
    if width is None:
        if tgt is None:
            raise ValueError("multi_aggr_bwd: an edge list needs tgt")
        tgt = _i32c(tgt, "tgt")
        E, M, width = int(tgt.numel()), int(tgt.numel()), 0
    else:
        E, M, tgt = 0, Nt * int(width), None
    if rev_ptr.numel() != Ns + 1 or rev_pos.numel() < M:
        raise ValueError(f"multi_aggr_bwd: the by-source index does not fit {M} positions over {Ns} sources")
    second = "var" in aggrs or "std" in aggrs
    coef = torch.empty((2 if second else 1, Nt, F), dtype=torch.float32, device=dev)      # c0 and c1: two floats per target row
    g_x = torch.empty((Ns, F), dtype=torch.float32, device=dev)
    _t = timer.record('multi_aggr_bwd', dev)
    with _on(dev):
        _lib.check(L.dmet_multi_aggr_bwd_f32(_ptr(x), _ptr(g_out), _ptr(count), _ptr(mean), _ptr(var), _ptr(amin),
                                             _ptr(amax), _ptr(tgt), rev_ptr.data_ptr(), _ptr(rev_pos), Nt, Ns, E, width, F,
                                             groups, code, _ptr(coef[0]), _ptr(coef[1]) if second else None, _ptr(g_x),
                                             _stream(dev)), "dmet_multi_aggr_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return g_x


WEIGHTED_SUM_MAX_F = 256            # features per row (include/dmet.h, "Weighted aggregation")
WEIGHTED_SUM_MAX_K = GRAVNET_MAX_K    # DMET_MAX_K: the width of a table


def weighted_sum_check_shapes(x: torch.Tensor, w: Optional[torch.Tensor], num_targets: int, num_sources: int,
                              width: Optional[int] = None, num_edges: Optional[int] = None) -> None:
    """The argument errors of the weighted-aggregation entries, raised from shapes alone (before any device is asked for).
    The graph has num_targets rows over num_sources sources; width: the table form's k (None: an edge list of num_edges
    entries, when that is known).  w: None, or one scalar per position."""
    if x.dim() != 2:
        raise ValueError(f"weighted_sum: x must be [Ns, F], got {tuple(x.shape)}")
    F = x.shape[1]
    if not 1 <= F <= WEIGHTED_SUM_MAX_F:
        raise ValueError(f"weighted_sum: F={F} features, supported 1..{WEIGHTED_SUM_MAX_F}")
    if width is not None and not 1 <= width <= WEIGHTED_SUM_MAX_K:
        raise ValueError(f"weighted_sum: k={width}, supported 1..{WEIGHTED_SUM_MAX_K}")
    if x.shape[0] != num_sources:
        raise ValueError(f"weighted_sum: the graph indexes {num_sources} sources, x has {x.shape[0]} rows")
    if num_targets < 0:
        raise ValueError(f"weighted_sum: {num_targets} target rows")
    if w is not None:
        M = num_targets * width if width is not None else num_edges
        if M is not None and w.numel() != M:
            raise ValueError(f"weighted_sum: edge_weight must hold one scalar per position ({M}), got {tuple(w.shape)}")


def _weighted_sum_fwd(x: torch.Tensor, w: Optional[torch.Tensor], idx: torch.Tensor, rowptr: Optional[torch.Tensor],
                      num_targets: int):
    """(out[Nt, F], count[Nt] int32): out_i = sum_e w_e x[src(e)] over a table (idx = nbr[Nt, k], rowptr None) or a
    grouped edge list (idx = src[E], rowptr[Nt+1]); w [positions] or None (weight 1).  See include/dmet.h,
    dmet_weighted_sum_fwd_f32.  Not public, like _multi_aggr_fwd: propagate.py is the caller."""
    Nt = int(num_targets)
    table = rowptr is None and idx.dim() == 2
    weighted_sum_check_shapes(x, w, Nt, x.shape[0], idx.shape[1] if table else None, None if table else idx.numel())
    dev = _require_device(x, w, idx, rowptr)
    L = _lib.load()
    x = _f32c(x, "x")
    w = None if w is None else _f32c(w, "edge_weight").reshape(-1)
    idx, rowptr, E, width, _M = _row_graph("weighted_sum", idx, rowptr, Nt)
    Ns, F = x.shape
    out = torch.empty((Nt, F), dtype=torch.float32, device=dev)
    count = torch.empty((Nt,), dtype=torch.int32, device=dev)
    _t = timer.record('weighted_sum_fwd', dev)
    with _on(dev):
        _lib.check(L.dmet_weighted_sum_fwd_f32(_ptr(x), _ptr(w), _ptr(idx), None if rowptr is None else rowptr.data_ptr(),
                                               Nt, Ns, E, width, F, _ptr(out), _ptr(count), _stream(dev)),
                   "dmet_weighted_sum_fwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, count


def _weighted_sum_bwd(g_out: torch.Tensor, x: torch.Tensor, w: Optional[torch.Tensor], idx: torch.Tensor,
                      rowptr: Optional[torch.Tensor], tgt: Optional[torch.Tensor], rev_ptr: Optional[torch.Tensor],
                      rev_pos: Optional[torch.Tensor], need_x: bool = True, need_w: bool = True):
    """(g_x[Ns, F] or None, g_w[positions] or None) of _weighted_sum_fwd; (rev_ptr, rev_pos) = the graph's by-source index
    (read only for g_x), tgt[E] names the row of every position of a list.  A pass nobody needs is not launched.  See
    include/dmet.h, dmet_weighted_sum_bwd_f32."""
    if not need_x and not need_w:
        return None, None
    Nt = int(g_out.shape[0])
    table = rowptr is None and idx.dim() == 2
    weighted_sum_check_shapes(x, w, Nt, x.shape[0], idx.shape[1] if table else None, None if table else idx.numel())
    Ns, F = x.shape
    if tuple(g_out.shape) != (Nt, F):
        raise ValueError(f"weighted_sum_bwd: g_out must be [{Nt}, {F}], got {tuple(g_out.shape)}")
    dev = _require_device(g_out, x, w, idx, rowptr, tgt, rev_ptr, rev_pos)
    L = _lib.load()
    x = _f32c(x, "x"); g_out = _f32c(g_out, "g_out")
    w = None if w is None else _f32c(w, "edge_weight").reshape(-1)
    idx, rowptr, E, width, M = _row_graph("weighted_sum", idx, rowptr, Nt)
    if rowptr is not None:
        if tgt is None or tgt.numel() != E:
            raise ValueError(f"weighted_sum_bwd: an edge list needs tgt [{E}]")
        tgt = _i32c(tgt, "tgt")
    else:
        tgt = None
    if need_x:
        if rev_ptr is None or rev_pos is None:
            raise ValueError("weighted_sum_bwd: g_x needs the by-source index")
        rev_ptr = _i32c(rev_ptr, "rev_ptr"); rev_pos = _i32c(rev_pos, "rev_pos")
        if rev_ptr.numel() != Ns + 1 or rev_pos.numel() < M:
            raise ValueError(f"weighted_sum_bwd: the by-source index does not fit {M} positions over {Ns} sources")
    else:
        rev_ptr = rev_pos = None
    g_x = torch.empty((Ns, F), dtype=torch.float32, device=dev) if need_x else None
    g_w = torch.empty((M,), dtype=torch.float32, device=dev) if need_w else None
    if (need_x and Ns > 0) or (need_w and M > 0):       # else both results are empty and a NULL pair is an argument error
        _t = timer.record('weighted_sum_bwd', dev)
        with _on(dev):
            _lib.check(L.dmet_weighted_sum_bwd_f32(_ptr(x), _ptr(w), _ptr(g_out), _ptr(idx),
                                                   None if rowptr is None else rowptr.data_ptr(), _ptr(tgt), _ptr(rev_ptr),
                                                   _ptr(rev_pos), Nt, Ns, E, width, F, _ptr(g_x), _ptr(g_w), _stream(dev)),
                       "dmet_weighted_sum_bwd_f32")
        if _t is not None:
            _t.record(torch.cuda.current_stream(dev))
    return g_x, g_w


ATTENTION_MAX_C = 64     # channels per head (include/dmet.h, "Attention aggregation")
ATTENTION_MAX_H = 16     # heads
ATTENTION_MAX_HC = 256   # heads * channels
ATTENTION_MAX_K = GRAVNET_MAX_K   # DMET_MAX_K: the width of a table, as for GravNet


def _row_softmax_limits(who: str, H: int, C: int, width: Optional[int]) -> None:
    """The ranges csrc/row_softmax.h's kernels take, for attention and GAT alike; width: a table's k (None: a list)."""
    if not 1 <= C <= ATTENTION_MAX_C:
        raise ValueError(f"{who}: C={C} channels per head, supported 1..{ATTENTION_MAX_C}")
    if not 1 <= H <= ATTENTION_MAX_H:
        raise ValueError(f"{who}: H={H} heads, supported 1..{ATTENTION_MAX_H}")
    if H * C > ATTENTION_MAX_HC:
        raise ValueError(f"{who}: H*C={H * C}, supported up to {ATTENTION_MAX_HC}")
    if width is not None and not 1 <= width <= ATTENTION_MAX_K:
        raise ValueError(f"{who}: k={width}, supported 1..{ATTENTION_MAX_K}")


def attention_check_shapes(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_targets: int, num_sources: int,
                           width: Optional[int] = None) -> None:
    """The argument errors of the attention entries, raised from shapes alone (before any device is asked for).  The graph
    has num_targets rows over num_sources sources; width: the table form's k (None: an edge list)."""
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError(f"attention: q [Nt, H, C], k and v [Ns, H, C] must be 3-D, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    H, C = q.shape[1], q.shape[2]
    _row_softmax_limits("attention", H, C, width)
    if tuple(k.shape[1:]) != (H, C) or tuple(v.shape[1:]) != (H, C):
        raise ValueError(f"attention: q has {H} heads of {C} channels, k {tuple(k.shape[1:])}, v {tuple(v.shape[1:])}")
    if k.shape[0] != v.shape[0]:
        raise ValueError(f"attention: k has {k.shape[0]} rows, v has {v.shape[0]}")
    if q.shape[0] != num_targets:
        raise ValueError(f"attention: the graph has {num_targets} target rows, q has {q.shape[0]}")
    if k.shape[0] != num_sources:
        raise ValueError(f"attention: the graph indexes {num_sources} sources, k and v have {k.shape[0]} rows")


def _row_graph(who: str, idx: torch.Tensor, rowptr: Optional[torch.Tensor], Nt: int):
    """(idx, rowptr, E, width, positions) of a table (rowptr None, idx = nbr[Nt, k]) or a list (idx = src[E])."""
    idx = _i32c(idx, "nbr" if rowptr is None else "src")
    if rowptr is None:
        if idx.dim() != 2 or idx.shape[0] != Nt:
            raise ValueError(f"{who}: nbr must be [{Nt}, k], got {tuple(idx.shape)}")
        return idx, None, 0, int(idx.shape[1]), Nt * int(idx.shape[1])
    rowptr = _i32c(rowptr, "rowptr")
    if idx.dim() != 1 or rowptr.numel() != Nt + 1:
        raise ValueError(f"{who}: src must be [E] and rowptr [{Nt + 1}], got {tuple(idx.shape)} and {tuple(rowptr.shape)}")
    return idx, rowptr, int(idx.numel()), 0, int(idx.numel())


def _row_softmax_bwd_args(who: str, g_out: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, rev_ptr: torch.Tensor,
                          rev_pos: torch.Tensor, rowptr: Optional[torch.Tensor], tgt: Optional[torch.Tensor], Nt: int,
                          Ns: int, H: int, C: int, E: int, M: int):
    """(rev_ptr, rev_pos, tgt) as the backward entries take them, once the row tensors, the by-source index and a list's
    tgt fit the graph."""
    rev_ptr = _i32c(rev_ptr, "rev_ptr"); rev_pos = _i32c(rev_pos, "rev_pos")
    if g_out.shape != (Nt, H, C) or out.shape != (Nt, H, C) or lse.shape != (Nt, H):
        raise ValueError(f"{who}: g_out and out must be [{Nt}, {H}, {C}] and lse [{Nt}, {H}]")
    if rev_ptr.numel() != Ns + 1 or rev_pos.numel() < M:
        raise ValueError(f"{who}: the by-source index does not fit {M} positions over {Ns} sources")
    if rowptr is not None:
        if tgt is None or tgt.numel() != E:
            raise ValueError(f"{who}: an edge list needs tgt [{E}]")
        tgt = _i32c(tgt, "tgt")
    return rev_ptr, rev_pos, tgt


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, idx: torch.Tensor, rowptr: Optional[torch.Tensor] = None,
                  want_alpha: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(out[Nt, H, C], lse[Nt, H], alpha[Nt*k or E, H] or None) of softmax attention over a table (idx = nbr[Nt, k],
    rowptr None) or a grouped edge list (idx = src[E], rowptr[Nt+1]); see include/dmet.h, dmet_attention_fwd_f32."""
    Nt, Ns = q.shape[0], k.shape[0]
    attention_check_shapes(q, k, v, Nt, Ns, idx.shape[1] if rowptr is None and idx.dim() == 2 else None)
    dev = _require_device(q, k, v, idx, rowptr)
    L = _lib.load()
    q = _f32c(q, "q"); k = _f32c(k, "k"); v = _f32c(v, "v")
    idx, rowptr, E, width, M = _row_graph("attention", idx, rowptr, Nt)
    _n, H, C = q.shape
    out = torch.empty((Nt, H, C), dtype=torch.float32, device=dev)
    lse = torch.empty((Nt, H), dtype=torch.float32, device=dev)
    alpha = torch.empty((M, H), dtype=torch.float32, device=dev) if want_alpha else None
    _t = timer.record('attention_fwd', dev)
    with _on(dev):
        _lib.check(L.dmet_attention_fwd_f32(q.data_ptr(), _ptr(k), _ptr(v), _ptr(idx), None if rowptr is None else
                                            rowptr.data_ptr(), Nt, Ns, E, width, H, C, out.data_ptr(), lse.data_ptr(),
                                            _ptr(alpha), _stream(dev)), "dmet_attention_fwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, lse, alpha


def attention_bwd(g_out: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor,
                  lse: torch.Tensor, idx: torch.Tensor, rev_ptr: torch.Tensor, rev_pos: torch.Tensor,
                  rowptr: Optional[torch.Tensor] = None,
                  tgt: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(g_q[Nt, H, C], g_k[Ns, H, C], g_v[Ns, H, C]) of attention_fwd; (rev_ptr, rev_pos) = the graph's by-source index
    (table.reverse() / EdgeList.by_source()), tgt = EdgeList.tgt for a list.  See include/dmet.h, dmet_attention_bwd_f32."""
    Nt, Ns = q.shape[0], k.shape[0]
    attention_check_shapes(q, k, v, Nt, Ns, idx.shape[1] if rowptr is None and idx.dim() == 2 else None)
    dev = _require_device(g_out, q, k, v, out, lse, idx, rev_ptr, rev_pos, rowptr, tgt)
    L = _lib.load()
    q = _f32c(q, "q"); k = _f32c(k, "k"); v = _f32c(v, "v"); out = _f32c(out, "out"); lse = _f32c(lse, "lse")
    g_out = _f32c(g_out, "g_out")
    idx, rowptr, E, width, M = _row_graph("attention", idx, rowptr, Nt)
    _n, H, C = q.shape
    rev_ptr, rev_pos, tgt = _row_softmax_bwd_args("attention_bwd", g_out, out, lse, rev_ptr, rev_pos, rowptr, tgt, Nt, Ns, H,
                                                  C, E, M)
    g_q = torch.empty((Nt, H, C), dtype=torch.float32, device=dev)
    g_kv = torch.empty((2, Ns, H, C), dtype=torch.float32, device=dev)
    work = torch.empty((2, M, H), dtype=torch.float32, device=dev)     # alpha and g_score: the per-edge buffers, 8 B per head
    _t = timer.record('attention_bwd', dev)
    with _on(dev):
        _lib.check(L.dmet_attention_bwd_f32(q.data_ptr(), _ptr(k), _ptr(v), out.data_ptr(), lse.data_ptr(), g_out.data_ptr(),
                                            _ptr(idx), None if rowptr is None else rowptr.data_ptr(), _ptr(tgt),
                                            rev_ptr.data_ptr(), rev_pos.data_ptr(), Nt, Ns, E, width, H, C,
                                            _ptr(work[0]), _ptr(work[1]), g_q.data_ptr(), _ptr(g_kv[0]), _ptr(g_kv[1]),
                                            _stream(dev)), "dmet_attention_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return g_q, g_kv[0], g_kv[1]


GAT_MAX_C = ATTENTION_MAX_C      # include/dmet.h, "GAT aggregation": the attention section's limits
GAT_MAX_H = ATTENTION_MAX_H
GAT_MAX_HC = ATTENTION_MAX_HC
GAT_MAX_K = ATTENTION_MAX_K
GAT_V1, GAT_V2 = 1, 2            # the ABI's mode: GATConv / GATv2Conv


def gat_check_shapes(mode: int, xl: torch.Tensor, a: torch.Tensor, b: torch.Tensor, num_targets: int, num_sources: int,
                     width: Optional[int] = None, negative_slope: float = 0.2, self_loops: bool = False) -> None:
    """The argument errors of the GAT entries, raised from shapes alone (before any device is asked for).  mode GAT_V2:
    (a, b) = (xr[Nt, H, C], att[H, C]); mode GAT_V1: (a, b) = (s_src[Ns, H], s_dst[Nt, H]).  The graph has num_targets
    rows over num_sources sources; width: the table form's k (None: an edge list)."""
    if mode not in (GAT_V1, GAT_V2):
        raise ValueError(f"gat: mode={mode!r}, {GAT_V1} (GATConv) or {GAT_V2} (GATv2Conv)")
    if xl.dim() != 3:
        raise ValueError(f"gat: xl must be [Ns, H, C], got {tuple(xl.shape)}")
    H, C = xl.shape[1], xl.shape[2]
    _row_softmax_limits("gat", H, C, width)
    slope = float(negative_slope)
    if not (math.isfinite(slope) and slope >= 0.0):
        raise ValueError(f"gat: negative_slope={negative_slope!r} must be finite and >= 0")
    if mode == GAT_V2:
        if a.dim() != 3 or tuple(a.shape[1:]) != (H, C):
            raise ValueError(f"gat: xl has {H} heads of {C} channels, xr must be [Nt, {H}, {C}], got {tuple(a.shape)}")
        if tuple(b.shape) not in ((H, C), (1, H, C)):
            raise ValueError(f"gat: att must be [{H}, {C}] (or [1, {H}, {C}]), got {tuple(b.shape)}")
        nt = a.shape[0]
    else:
        if a.dim() != 2 or a.shape[1] != H or a.shape[0] != xl.shape[0]:
            raise ValueError(f"gat: s_src must be [{xl.shape[0]}, {H}], got {tuple(a.shape)}")
        if b.dim() != 2 or b.shape[1] != H:
            raise ValueError(f"gat: s_dst must be [Nt, {H}], got {tuple(b.shape)}")
        nt = b.shape[0]
    if nt != num_targets:
        raise ValueError(f"gat: the graph has {num_targets} target rows, {'xr' if mode == GAT_V2 else 's_dst'} has {nt}")
    if xl.shape[0] != num_sources:
        raise ValueError(f"gat: the graph indexes {num_sources} sources, xl has {xl.shape[0]} rows")
    if self_loops and num_targets != num_sources:
        raise ValueError(f"gat: self_loops needs one node set, the graph has {num_targets} targets over {num_sources} "
                         "sources; pass self_loops=False")


def _gat_operands(mode, xl, a, b):
    """(xr, att, s_src, s_dst) as the ABI takes them, fp32 contiguous; the other mode's pair is None."""
    if mode == GAT_V2:
        return _f32c(a, "xr"), _f32c(b.reshape(xl.shape[1], xl.shape[2]), "att"), None, None
    return None, None, _f32c(a, "s_src"), _f32c(b, "s_dst")


def _gat_fwd(mode: int, xl: torch.Tensor, a: torch.Tensor, b: torch.Tensor, idx: torch.Tensor,
              rowptr: Optional[torch.Tensor] = None, negative_slope: float = 0.2, self_loops: bool = False,
             want_alpha: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(out[Nt, H, C], lse[Nt, H], alpha[Nt*k or E, H] or None) of additive attention over a table (idx = nbr[Nt, k],
    rowptr None) or a grouped edge list (idx = src[E], rowptr[Nt+1]).  mode GAT_V2: (a, b) = (xr, att); GAT_V1: (a, b) =
    (s_src, s_dst).  See include/dmet.h, dmet_gat_fwd_f32.  Not public, like _pointnet_fwd: the closed table of allocating
    wrappers names the public ones; gat.py is the caller."""
    Ns = xl.shape[0]
    Nt = (a if mode == GAT_V2 else b).shape[0]
    gat_check_shapes(mode, xl, a, b, Nt, Ns, idx.shape[1] if rowptr is None and idx.dim() == 2 else None, negative_slope,
                     self_loops)
    dev = _require_device(xl, a, b, idx, rowptr)
    L = _lib.load()
    xl = _f32c(xl, "xl")
    xr, att, s_src, s_dst = _gat_operands(mode, xl, a, b)
    idx, rowptr, E, width, M = _row_graph("gat", idx, rowptr, Nt)
    _n, H, C = xl.shape
    out = torch.empty((Nt, H, C), dtype=torch.float32, device=dev)
    lse = torch.empty((Nt, H), dtype=torch.float32, device=dev)
    alpha = torch.empty((M, H), dtype=torch.float32, device=dev) if want_alpha else None
    _t = timer.record('gat_fwd', dev)
    with _on(dev):
        _lib.check(L.dmet_gat_fwd_f32(mode, _ptr(xl), _ptr(xr), _ptr(att), _ptr(s_src), _ptr(s_dst), float(negative_slope),
                                      int(bool(self_loops)), _ptr(idx), None if rowptr is None else rowptr.data_ptr(),
                                      Nt, Ns, E, width, H, C, out.data_ptr(), lse.data_ptr(), _ptr(alpha), _stream(dev)),
                   "dmet_gat_fwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, lse, alpha


def _gat_bwd(mode: int, g_out: torch.Tensor, xl: torch.Tensor, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor,
             lse: torch.Tensor, idx: torch.Tensor, rev_ptr: torch.Tensor, rev_pos: torch.Tensor,
             rowptr: Optional[torch.Tensor] = None, tgt: Optional[torch.Tensor] = None, negative_slope: float = 0.2,
             self_loops: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Gradients of _gat_fwd.  mode GAT_V2: (g_xl[Ns, H, C], g_xr[Nt, H, C], g_att[H, C]); mode GAT_V1: (g_xl[Ns, H, C],
    g_s_src[Ns, H], g_s_dst[Nt, H]).  (rev_ptr, rev_pos) = the graph's by-source index (table.reverse() /
    EdgeList.by_source()), tgt = EdgeList.tgt for a list.  g_att is the sum over the targets of the kernel's per-target
    rows, one torch.sum.  See include/dmet.h, dmet_gat_bwd_f32."""
    Ns = xl.shape[0]
    Nt = (a if mode == GAT_V2 else b).shape[0]
    gat_check_shapes(mode, xl, a, b, Nt, Ns, idx.shape[1] if rowptr is None and idx.dim() == 2 else None, negative_slope,
                     self_loops)
    dev = _require_device(g_out, xl, a, b, out, lse, idx, rev_ptr, rev_pos, rowptr, tgt)
    L = _lib.load()
    xl = _f32c(xl, "xl"); out = _f32c(out, "out"); lse = _f32c(lse, "lse"); g_out = _f32c(g_out, "g_out")
    xr, att, s_src, s_dst = _gat_operands(mode, xl, a, b)
    idx, rowptr, E, width, M = _row_graph("gat", idx, rowptr, Nt)
    _n, H, C = xl.shape
    rev_ptr, rev_pos, tgt = _row_softmax_bwd_args("gat_bwd", g_out, out, lse, rev_ptr, rev_pos, rowptr, tgt, Nt, Ns, H, C, E, M)
    g_xl = torch.empty((Ns, H, C), dtype=torch.float32, device=dev)
    work = torch.empty((2, M, H), dtype=torch.float32, device=dev)     # alpha and g_score: the per-edge buffers, 8 B per head
    work_self = torch.empty((2, Nt, H), dtype=torch.float32, device=dev) if self_loops else None
    g_xr = g_rows = g_ssrc = g_sdst = None
    if mode == GAT_V2:
        g_t = torch.empty((2, Nt, H, C), dtype=torch.float32, device=dev)      # g_xr and the per-target rows of g_att
        g_xr, g_rows = g_t[0], g_t[1]
    else:
        g_ssrc = torch.empty((Ns, H), dtype=torch.float32, device=dev)
        g_sdst = torch.empty((Nt, H), dtype=torch.float32, device=dev)
    _t = timer.record('gat_bwd', dev)
    with _on(dev):
        _lib.check(L.dmet_gat_bwd_f32(mode, _ptr(xl), _ptr(xr), _ptr(att), _ptr(s_src), _ptr(s_dst), float(negative_slope),
                                      int(bool(self_loops)), out.data_ptr(), lse.data_ptr(), g_out.data_ptr(), _ptr(idx),
                                      None if rowptr is None else rowptr.data_ptr(), _ptr(tgt), rev_ptr.data_ptr(),
                                      rev_pos.data_ptr(), Nt, Ns, E, width, H, C, _ptr(work[0]), _ptr(work[1]),
                                      None if work_self is None else _ptr(work_self[0]),
                                      None if work_self is None else _ptr(work_self[1]), _ptr(g_xl), _ptr(g_xr),
                                      _ptr(g_rows), _ptr(g_ssrc), _ptr(g_sdst), _stream(dev)), "dmet_gat_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    if mode == GAT_V2:
        return g_xl, g_xr, g_rows.sum(0)
    return g_xl, g_ssrc, g_sdst


POINTNET_MAX_F = 128       # include/dmet.h, "PointNet convolution"
POINTNET_MAX_D = 8
POINTNET_MAX_H1 = 128
POINTNET_H2 = (16, 32, 64, 128)
POINTNET_MAX_WIDTH = 1024  # DMET_POINTNET_MAX_WIDTH
POINTNET_ACT = {"relu": 0, "elu": 1}


def pointnet_widths_supported(F: int, D: int, H1: int, H2: int) -> bool:
    """What dmet_pointnet_supported answers, from the widths alone (no library, no device)."""
    return 0 <= F <= POINTNET_MAX_F and 1 <= D <= POINTNET_MAX_D and 1 <= H1 <= POINTNET_MAX_H1 and H2 in POINTNET_H2


def pointnet_check_shapes(x_src: Optional[torch.Tensor], pos_src: torch.Tensor, pos_dst: torch.Tensor, W1: torch.Tensor,
                          b1: Optional[torch.Tensor], W2: torch.Tensor, b2: Optional[torch.Tensor], act: str,
                          num_targets: int, num_sources: int, width: Optional[int], self_loop: bool) -> None:
    """The argument errors of the PointNet entries, raised from shapes alone (before any device is asked for).  The graph
    has num_targets rows over num_sources sources; width: the table form's (None: an edge list)."""
    if pos_src.dim() != 2 or pos_dst.dim() != 2 or pos_src.shape[1] != pos_dst.shape[1]:
        raise ValueError(f"pointnet: pos_src [Ns, D] and pos_dst [Nt, D] must be 2-D with one D, got {tuple(pos_src.shape)} "
                         f"and {tuple(pos_dst.shape)}")
    if x_src is not None and (x_src.dim() != 2 or x_src.shape[0] != pos_src.shape[0]):
        raise ValueError(f"pointnet: x_src must be [{pos_src.shape[0]}, F], got {tuple(x_src.shape)}")
    F, D = (0 if x_src is None else x_src.shape[1]), pos_src.shape[1]
    if W1.dim() != 2 or W2.dim() != 2 or W1.shape[1] != F + D or W2.shape[1] != W1.shape[0]:
        raise ValueError(f"pointnet: W1 must be [H1, F + D = {F + D}] and W2 [H2, H1], got {tuple(W1.shape)} and "
                         f"{tuple(W2.shape)}")
    H1, H2 = W1.shape[0], W2.shape[0]
    if not pointnet_widths_supported(F, D, H1, H2):
        raise ValueError(f"pointnet: unsupported widths F={F}, D={D}, H1={H1}, H2={H2}: 0 <= F <= {POINTNET_MAX_F}, "
                         f"1 <= D <= {POINTNET_MAX_D}, 1 <= H1 <= {POINTNET_MAX_H1}, H2 in {POINTNET_H2}")
    if (b1 is not None and b1.numel() != H1) or (b2 is not None and b2.numel() != H2):
        raise ValueError(f"pointnet: b1 must hold H1 = {H1} and b2 H2 = {H2} elements")
    if act not in POINTNET_ACT:
        raise ValueError(f"pointnet: act must be one of {sorted(POINTNET_ACT)}, got {act!r}")
    if width is not None and not 1 <= width <= POINTNET_MAX_WIDTH:
        raise ValueError(f"pointnet: table width {width}, supported 1..{POINTNET_MAX_WIDTH}")
    if pos_dst.shape[0] != num_targets:
        raise ValueError(f"pointnet: the graph has {num_targets} target rows, pos_dst has {pos_dst.shape[0]}")
    if pos_src.shape[0] != num_sources:
        raise ValueError(f"pointnet: the graph indexes {num_sources} sources, pos_src has {pos_src.shape[0]} rows")
    if self_loop and num_targets != num_sources:
        raise ValueError(f"pointnet: self loops need one node set, got {num_sources} sources and {num_targets} targets")


def _pointnet_graph(idx: torch.Tensor, rowptr: Optional[torch.Tensor], cnt: Optional[torch.Tensor], Nt: int):
    """(idx, rowptr, cnt, E, width, positions) of a table (rowptr None, idx = nbr[Nt, width]) or a list (idx = src[E])."""
    idx = _i32c(idx, "nbr" if rowptr is None else "src")
    if rowptr is None:
        if idx.dim() != 2 or idx.shape[0] != Nt:
            raise ValueError(f"pointnet: nbr must be [{Nt}, width], got {tuple(idx.shape)}")
        if cnt is not None:
            cnt = _i32c(cnt, "cnt")
            if cnt.numel() != Nt:
                raise ValueError(f"pointnet: cnt must hold {Nt} entries, got {cnt.numel()}")
        return idx, None, cnt, 0, int(idx.shape[1]), Nt * int(idx.shape[1])
    rowptr = _i32c(rowptr, "rowptr")
    if idx.dim() != 1 or rowptr.numel() != Nt + 1:
        raise ValueError(f"pointnet: src must be [E] and rowptr [{Nt + 1}], got {tuple(idx.shape)} and {tuple(rowptr.shape)}")
    return idx, rowptr, None, int(idx.numel()), 0, int(idx.numel())


def _pointnet_fwd(x_src: Optional[torch.Tensor], pos_src: torch.Tensor, pos_dst: torch.Tensor, idx: torch.Tensor,
                  rowptr: Optional[torch.Tensor], cnt: Optional[torch.Tensor], W1: torch.Tensor, b1: Optional[torch.Tensor],
                  W2: torch.Tensor, b2: Optional[torch.Tensor], act: str, act2: bool, self_loop: bool):
    """(out[Nt, H2], win[Nt, H2] int32, state) of the fused PointNet aggregation over a table (idx = nbr[Nt, width], rowptr
    None, cnt optional) or a grouped edge list (idx = src[E], rowptr[Nt+1]); see include/dmet.h, dmet_pointnet_fwd_f32.
    `state` = (a, b, s or None) is what _pointnet_bwd needs beside out and win.  Not public: the closed table of
    allocating wrappers names the public ones; pointnet.py is the caller."""
    Nt, Ns = pos_dst.shape[0], pos_src.shape[0]
    width = idx.shape[1] if rowptr is None and idx.dim() == 2 else None
    pointnet_check_shapes(x_src, pos_src, pos_dst, W1, b1, W2, b2, act, Nt, Ns, width, self_loop)
    dev = _require_device(x_src, pos_src, pos_dst, idx, rowptr, cnt, W1, b1, W2, b2)
    L = _lib.load()
    same = pos_src is pos_dst
    pos_src = _f32c(pos_src, "pos_src")
    pos_dst = pos_src if same else _f32c(pos_dst, "pos_dst")
    if x_src is not None:
        x_src = _f32c(x_src, "x_src")
    W1 = _f32c(W1, "W1"); W2 = _f32c(W2, "W2")
    b1 = None if b1 is None else _f32c(b1, "b1")
    b2 = None if b2 is None else _f32c(b2, "b2")
    idx, rowptr, cnt, E, width, _M = _pointnet_graph(idx, rowptr, cnt, Nt)
    F, D = (0 if x_src is None else x_src.shape[1]), pos_src.shape[1]
    H1, H2 = W1.shape[0], W2.shape[0]
    out = torch.empty((Nt, H2), dtype=torch.float32, device=dev)
    win = torch.empty((Nt, H2), dtype=torch.int32, device=dev)
    a = torch.empty((Ns, H1), dtype=torch.float32, device=dev)
    b = torch.empty((Nt, H1), dtype=torch.float32, device=dev)
    s = torch.empty((Nt, H1), dtype=torch.float32, device=dev) if self_loop else None
    _t = timer.record('pointnet_fwd', dev)
    with _on(dev):
        ws = _ws(L.dmet_pointnet_workspace_bytes(F, D, H1, H2), dev)
        _lib.check(L.dmet_pointnet_fwd_f32(_ptr(x_src), _ptr(pos_src), _ptr(pos_dst), _ptr(idx),
                                           None if rowptr is None else rowptr.data_ptr(), _ptr(cnt), Nt, Ns, E, width, F, D,
                                           W1.data_ptr(), _ptr(b1), H1, W2.data_ptr(), _ptr(b2), H2, POINTNET_ACT[act],
                                           1 if act2 else 0, 1 if self_loop else 0, _ptr(a), _ptr(b), _ptr(s), _ptr(out),
                                           _ptr(win), ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_pointnet_fwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, win, (a, b, s)


def _pointnet_bwd(g_out: torch.Tensor, out: torch.Tensor, win: torch.Tensor, state, x_src: Optional[torch.Tensor],
                  pos_src: torch.Tensor, pos_dst: torch.Tensor, idx: torch.Tensor, rev_ptr: torch.Tensor,
                  rev_pos: torch.Tensor, rowptr: Optional[torch.Tensor], tgt: Optional[torch.Tensor],
                  cnt: Optional[torch.Tensor], W1: torch.Tensor, W2: torch.Tensor, act: str, act2: bool, self_loop: bool,
                  want=(True, True, True, True, True, True, True)):
    """(g_x, g_pos_src, g_pos_dst, g_W1, g_b1, g_W2, g_b2) of _pointnet_fwd, None where `want` says so (g_x also for
    F == 0); (rev_ptr, rev_pos) = the graph's by-source index (table.reverse() / EdgeList.by_source()), tgt = EdgeList.tgt
    for a list.  See include/dmet.h, dmet_pointnet_bwd_f32.  g_W1 and g_b1 are formed here through dmet_xty_f32."""
    a, b, s = state
    Nt, Ns = b.shape[0], a.shape[0]
    dev = _require_device(g_out, out, win, a, b, s, idx, rev_ptr, rev_pos, rowptr, tgt, cnt, W1, W2)
    L = _lib.load()
    g_out = _f32c(g_out, "g_out"); W1 = _f32c(W1, "W1"); W2 = _f32c(W2, "W2")
    idx, rowptr, cnt, E, width, M = _pointnet_graph(idx, rowptr, cnt, Nt)
    rev_ptr = _i32c(rev_ptr, "rev_ptr"); rev_pos = _i32c(rev_pos, "rev_pos")
    H1, H2 = W1.shape[0], W2.shape[0]
    D = pos_src.shape[1]
    F = W1.shape[1] - D
    if tuple(g_out.shape) != (Nt, H2) or tuple(out.shape) != (Nt, H2) or tuple(win.shape) != (Nt, H2):
        raise ValueError(f"pointnet_bwd: g_out, out and win must be [{Nt}, {H2}]")
    if rev_ptr.numel() != Ns + 1:
        raise ValueError(f"pointnet_bwd: the by-source index must cover {Ns} sources")
    if rowptr is not None:
        if tgt is None or tgt.numel() != E:
            raise ValueError(f"pointnet_bwd: an edge list needs tgt [{E}]")
        tgt = _i32c(tgt, "tgt")
    want_x, want_ps, want_pd, want_w1, want_b1, want_w2, want_b2 = want
    g_a = torch.empty((Ns, H1), dtype=torch.float32, device=dev)
    g_b = torch.empty((Nt, H1), dtype=torch.float32, device=dev)
    g_s = torch.empty((Nt, H1), dtype=torch.float32, device=dev) if self_loop else None
    g_x = torch.empty((Ns, F), dtype=torch.float32, device=dev) if want_x and F > 0 else None
    g_ps = torch.empty((Ns, D), dtype=torch.float32, device=dev) if want_ps else None
    g_pd = torch.empty((Nt, D), dtype=torch.float32, device=dev) if want_pd else None
    g_W2 = torch.empty((H2, H1), dtype=torch.float32, device=dev) if want_w2 else None
    g_b2 = torch.empty((H2,), dtype=torch.float32, device=dev) if want_b2 else None
    _t = timer.record('pointnet_bwd', dev)
    with _on(dev):
        ws = _ws(L.dmet_pointnet_workspace_bytes(F, D, H1, H2), dev)
        _lib.check(L.dmet_pointnet_bwd_f32(_ptr(a), _ptr(b), _ptr(s), _ptr(out), _ptr(win), _ptr(g_out), _ptr(idx),
                                           None if rowptr is None else rowptr.data_ptr(), _ptr(tgt), _ptr(cnt),
                                           rev_ptr.data_ptr(), rev_pos.data_ptr(), Nt, Ns, E, width, F, D, W1.data_ptr(), H1,
                                           W2.data_ptr(), H2, POINTNET_ACT[act], 1 if act2 else 0, 1 if self_loop else 0,
                                           _ptr(g_a), _ptr(g_b), _ptr(g_s), _ptr(g_x), _ptr(g_ps), _ptr(g_pd), _ptr(g_W2),
                                           _ptr(g_b2), ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_pointnet_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    g_W1 = g_b1 = None
    if want_w1 or want_b1:
        g_as = g_a + g_s if self_loop else g_a        # what reaches x and b1: the implicit entry reads no position
        if want_b1:
            g_b1 = xty_wide_ones(g_as) if Ns else torch.zeros((H1,), dtype=torch.float32, device=dev)
        if want_w1:
            parts = []
            if F > 0:
                parts.append(_xty_wide(g_as, _f32c(x_src, "x_src")) if Ns else torch.zeros((H1, F), dtype=torch.float32,
                                                                                          device=dev))
            gp = torch.zeros((H1, D), dtype=torch.float32, device=dev)
            if Ns:
                gp = gp + _xty_wide(g_a, _f32c(pos_src, "pos_src"))
            if Nt:
                gp = gp + _xty_wide(g_b, _f32c(pos_dst, "pos_dst"))
            parts.append(gp)
            g_W1 = torch.cat(parts, dim=1)
    return g_x, g_ps, g_pd, g_W1, g_b1, g_W2, g_b2


def reverse_index(keys: torch.Tensor, num_keys: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable sort of positions by int32 key: rev_ptr[num_keys+1] int32, rev_pos[M] int32 (see include/dmet.h)."""
    dev = _require_device(keys)
    L = _lib.load()
    if keys.dtype != torch.int32 or not keys.is_contiguous():
        raise TypeError("keys must be a contiguous int32 tensor")
    M = keys.numel()
    rev_ptr = torch.empty((num_keys + 1,), dtype=torch.int32, device=dev)
    # M == 0: no position exists; one element, zero, so that callers hold a tensor with an address (no output of the entry)
    rev_pos = torch.empty((M,), dtype=torch.int32, device=dev) if M else torch.zeros((1,), dtype=torch.int32, device=dev)
    _t = timer.record('reverse_index', dev)
    with _on(dev):
        ws = _ws(L.dmet_reverse_index_workspace_bytes(M, num_keys), dev)
        _lib.check(L.dmet_reverse_index(keys.data_ptr(), M, num_keys, rev_ptr.data_ptr(), rev_pos.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_reverse_index")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return rev_ptr, rev_pos


# ---- K2 / K3 un-fused ------------------------------------------------------------------------------------------
def edge_features(x: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    dev = _require_device(x, src, tgt)
    L = _lib.load()
    x = _f32a(x, "x")
    E = src.numel()
    H = x.shape[1]
    feat = torch.empty((E, 2 * H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_edge_features_f32(x.data_ptr(), src.data_ptr(), tgt.data_ptr(), E, H, feat.data_ptr(),
                                            _stream(dev)), "dmet_edge_features_f32")
    return feat


def edge_features_bwd(g_feat: torch.Tensor, rowptr: torch.Tensor, srcptr: torch.Tensor, srcperm: torch.Tensor,
                      N: int, H: int) -> torch.Tensor:
    dev = _require_device(g_feat, rowptr, srcptr, srcperm)
    L = _lib.load()
    g_feat = _f32c(g_feat, "g_feat")
    gx = torch.empty((N, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_edge_features_bwd_f32(g_feat.data_ptr(), rowptr.data_ptr(), srcptr.data_ptr(),
                                                srcperm.data_ptr(), N, H, gx.data_ptr(), _stream(dev)),
                   "dmet_edge_features_bwd_f32")
    return gx


def edge_features_xy(x_src: torch.Tensor, x_dst: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """feat[e] = [x_dst[tgt[e]] || x_src[src[e]] - x_dst[tgt[e]]]; the ids must be in range (dmet_edge_features_xy_f32)."""
    dev = _require_device(x_src, x_dst, src, tgt)
    L = _lib.load()
    x_src, x_dst = _f32c(x_src, "x_src"), _f32c(x_dst, "x_dst")
    E = src.numel()
    H = x_dst.shape[1]
    feat = torch.empty((E, 2 * H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_edge_features_xy_f32(x_src.data_ptr(), x_dst.data_ptr(), src.data_ptr(), tgt.data_ptr(), E, H,
                                               feat.data_ptr(), _stream(dev)), "dmet_edge_features_xy_f32")
    return feat


def edge_features_xy_bwd(g_feat: torch.Tensor, rowptr: torch.Tensor, srcptr: torch.Tensor, srcperm: torch.Tensor,
                         N_src: int, N_dst: int, H: int, want_src: bool = True, want_dst: bool = True):
    """(g_x_src [N_src, H] or None, g_x_dst [N_dst, H] or None) of edge_features_xy (dmet_edge_features_xy_bwd_f32)."""
    dev = _require_device(g_feat, rowptr, srcptr, srcperm)
    L = _lib.load()
    g_feat = _f32c(g_feat, "g_feat")
    g_src = torch.empty((N_src, H), dtype=torch.float32, device=dev) if want_src else None
    g_dst = torch.empty((N_dst, H), dtype=torch.float32, device=dev) if want_dst else None
    with _on(dev):
        _lib.check(L.dmet_edge_features_xy_bwd_f32(g_feat.data_ptr(), rowptr.data_ptr(), srcptr.data_ptr(),
                                                   srcperm.data_ptr(), N_src, N_dst, H,
                                                   g_src.data_ptr() if want_src else None,
                                                   g_dst.data_ptr() if want_dst else None, _stream(dev)),
                   "dmet_edge_features_xy_bwd_f32")
    return g_src, g_dst


def segment_max(msg: torch.Tensor, rowptr: torch.Tensor, N: int) -> Tuple[torch.Tensor, torch.Tensor]:
    dev = _require_device(msg, rowptr)
    L = _lib.load()
    msg = _f32c(msg, "msg")
    H = msg.shape[1]
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    arg = torch.empty((N, H), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_segment_max_f32(msg.data_ptr(), rowptr.data_ptr(), N, H, out.data_ptr(), arg.data_ptr(),
                                          _stream(dev)), "dmet_segment_max_f32")
    return out, arg


def segment_sum(msg: torch.Tensor, rowptr: torch.Tensor, N: int) -> torch.Tensor:
    dev = _require_device(msg, rowptr)
    L = _lib.load()
    msg = _f32c(msg, "msg")
    H = msg.shape[1]
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_segment_sum_f32(msg.data_ptr(), rowptr.data_ptr(), N, H, out.data_ptr(), _stream(dev)),
                   "dmet_segment_sum_f32")
    return out


def segment_max_bwd(g_out: torch.Tensor, arg: torch.Tensor, rowptr: torch.Tensor, E: int) -> torch.Tensor:
    dev = _require_device(g_out, arg, rowptr)
    L = _lib.load()
    g_out = _f32c(g_out, "g_out")
    N, H = g_out.shape
    g_msg = torch.empty((E, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_segment_max_bwd_f32(g_out.data_ptr(), arg.data_ptr(), rowptr.data_ptr(), N, H,
                                              g_msg.data_ptr(), _stream(dev)), "dmet_segment_max_bwd_f32")
    return g_msg


def segment_sum_bwd(g_out: torch.Tensor, rowptr: torch.Tensor, E: int) -> torch.Tensor:
    dev = _require_device(g_out, rowptr)
    L = _lib.load()
    g_out = _f32c(g_out, "g_out")
    N, H = g_out.shape
    g_msg = torch.empty((E, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_segment_sum_bwd_f32(g_out.data_ptr(), rowptr.data_ptr(), N, H, g_msg.data_ptr(),
                                              _stream(dev)), "dmet_segment_sum_bwd_f32")
    return g_msg


# ---- csrc/segment.hip: rows of any length; `max_len` is the hint of the longest row (0: unknown) ------------------------------
def _segment_args(src: torch.Tensor, rowptr: torch.Tensor, name: str):
    dev = _require_device(src, rowptr)
    src = _f32c(src, name)
    if src.dim() != 2:
        raise ValueError(f"{name} must be [E, H], got {tuple(src.shape)}")
    if rowptr.dtype != torch.int32 or not rowptr.is_contiguous():
        raise TypeError("rowptr must be contiguous int32")
    return dev, src, rowptr.numel() - 1


def _segment_mean(src: torch.Tensor, rowptr: torch.Tensor, max_len: int = 0) -> torch.Tensor:
    dev, src, n = _segment_args(src, rowptr, "src")
    E, H = src.shape
    out = torch.empty((n, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_segment_mean_f32(src.data_ptr(), rowptr.data_ptr(), n, E, H, int(max_len), out.data_ptr(),
                                                     _stream(dev)), "dmet_segment_mean_f32")
    return out


def _segment_mean_bwd(g_out: torch.Tensor, rowptr: torch.Tensor, E: int, max_len: int = 0) -> torch.Tensor:
    dev, g_out, n = _segment_args(g_out, rowptr, "g_out")
    H = g_out.shape[1]
    g_src = torch.empty((E, H), dtype=torch.float32, device=dev) if n > 0 else torch.zeros((E, H), dtype=torch.float32,
                                                                                          device=dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_segment_mean_bwd_f32(g_out.data_ptr(), rowptr.data_ptr(), n, E, H, int(max_len),
                                                         g_src.data_ptr(), _stream(dev)), "dmet_segment_mean_bwd_f32")
    return g_src


def _segment_min(src: torch.Tensor, rowptr: torch.Tensor, max_len: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    dev, src, n = _segment_args(src, rowptr, "src")
    E, H = src.shape
    out = torch.empty((n, H), dtype=torch.float32, device=dev)
    arg = torch.empty((n, H), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_segment_min_f32(src.data_ptr(), rowptr.data_ptr(), n, E, H, int(max_len), out.data_ptr(),
                                                    arg.data_ptr(), _stream(dev)), "dmet_segment_min_f32")
    return out, arg


def _segment_softmax_fwd(src: torch.Tensor, rowptr: torch.Tensor, log: bool = False,
                         max_len: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y[E,H], lse[n,H]): the softmax (log: the log_softmax) of every row, and m + logf(l) per row."""
    dev, src, n = _segment_args(src, rowptr, "src")
    E, H = src.shape
    y = torch.empty((E, H), dtype=torch.float32, device=dev) if n > 0 else torch.zeros((E, H), dtype=torch.float32, device=dev)
    lse = torch.empty((n, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_segment_softmax_fwd_f32(src.data_ptr(), rowptr.data_ptr(), n, E, H, int(bool(log)),
                                                            int(max_len), y.data_ptr(), lse.data_ptr(), _stream(dev)),
                   "dmet_segment_softmax_fwd_f32")
    return y, lse


def _segment_softmax_bwd(y: torch.Tensor, g: torch.Tensor, rowptr: torch.Tensor, log: bool = False,
                         max_len: int = 0) -> torch.Tensor:
    dev, y, n = _segment_args(y, rowptr, "y")
    g = _f32c(g, "g")
    if g.shape != y.shape or g.device != dev:
        raise ValueError(f"g must be {tuple(y.shape)} on {dev}, got {tuple(g.shape)} on {g.device}")
    E, H = y.shape
    g_src = torch.empty((E, H), dtype=torch.float32, device=dev) if n > 0 else torch.zeros((E, H), dtype=torch.float32,
                                                                                          device=dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_segment_softmax_bwd_f32(y.data_ptr(), g.data_ptr(), rowptr.data_ptr(), n, E, H,
                                                            int(bool(log)), int(max_len), g_src.data_ptr(), _stream(dev)),
                   "dmet_segment_softmax_bwd_f32")
    return g_src


def _segment_logsumexp(src: torch.Tensor, rowptr: torch.Tensor, max_len: int = 0) -> torch.Tensor:
    dev, src, n = _segment_args(src, rowptr, "src")
    E, H = src.shape
    out = torch.empty((n, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_segment_logsumexp_f32(src.data_ptr(), rowptr.data_ptr(), n, E, H, int(max_len),
                                                          out.data_ptr(), _stream(dev)), "dmet_segment_logsumexp_f32")
    return out


def _segment_logsumexp_bwd(src: torch.Tensor, out: torch.Tensor, g_out: torch.Tensor, rowptr: torch.Tensor,
                           max_len: int = 0) -> torch.Tensor:
    dev, src, n = _segment_args(src, rowptr, "src")
    out, g_out = _f32c(out, "out"), _f32c(g_out, "g_out")
    E, H = src.shape
    if out.shape != (n, H) or g_out.shape != (n, H) or out.device != dev or g_out.device != dev:
        raise ValueError(f"out and g_out must be [{n}, {H}] on {dev}")
    g_src = torch.empty((E, H), dtype=torch.float32, device=dev) if n > 0 else torch.zeros((E, H), dtype=torch.float32,
                                                                                          device=dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_segment_logsumexp_bwd_f32(src.data_ptr(), out.data_ptr(), g_out.data_ptr(),
                                                              rowptr.data_ptr(), n, E, H, int(max_len), g_src.data_ptr(),
                                                              _stream(dev)), "dmet_segment_logsumexp_bwd_f32")
    return g_src


# ---- csrc/event_norm.hip: per-event column statistics and the elementwise pass of the normalisation layers -----------------
def _event_args(x: torch.Tensor, rowptr: torch.Tensor, name: str, *coef: Optional[torch.Tensor]):
    """(device, x, B) for fp32 rows x[N, F] grouped by rowptr[B+1]; every given `coef` must be a contiguous fp32 [B, F]."""
    dev, x, B = _segment_args(x, rowptr, name)
    for t in coef:
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (B, x.shape[1]) or not t.is_contiguous()
                              or t.device != dev):
            raise ValueError(f"per-event operands must be contiguous float32 [{B}, {x.shape[1]}] on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    return dev, x, B


def _event_moments(x: torch.Tensor, rowptr: torch.Tensor, max_len: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean[B, F], var[B, F]) of the rows of every event; see include/dmet.h, dmet_event_moments_f32."""
    dev, x, B = _event_args(x, rowptr, "x")
    N, F = x.shape
    mean = torch.empty((B, F), dtype=torch.float32, device=dev)
    var = torch.empty((B, F), dtype=torch.float32, device=dev)
    _t = timer.record('event_moments', dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_event_moments_f32(_ptr(x), rowptr.data_ptr(), B, N, F, int(max_len), _ptr(mean), _ptr(var),
                                                      _stream(dev)), "dmet_event_moments_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return mean, var


def _event_dots(g: torch.Tensor, x: Optional[torch.Tensor], rowptr: torch.Tensor, shift: Optional[torch.Tensor] = None,
                scale: Optional[torch.Tensor] = None, max_len: int = 0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(s1[B, F], s2[B, F]): the sums of g and of g * ((x - shift) * scale) over every event; x None: (s1, None)."""
    dev, g, B = _event_args(g, rowptr, "g", shift, scale)
    N, F = g.shape
    dots = x is not None
    if dots:
        x = _f32c(x, "x")
        if x.shape != g.shape or x.device != dev or shift is None or scale is None:
            raise ValueError(f"x must be {tuple(g.shape)} on {dev} and come with shift and scale")
    s1 = torch.empty((B, F), dtype=torch.float32, device=dev)
    s2 = torch.empty((B, F), dtype=torch.float32, device=dev) if dots else None
    _t = timer.record('event_dots', dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_event_dots_f32(_ptr(g), _ptr(x) if dots else None, rowptr.data_ptr(), B, N, F, int(max_len),
                                                   shift.data_ptr() if dots else None, scale.data_ptr() if dots else None,
                                                   _ptr(s1), s2.data_ptr() if dots else None, _stream(dev)),
                   "dmet_event_dots_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return s1, s2


def _event_affine(x: torch.Tensor, rowptr: torch.Tensor, shift: torch.Tensor, k1: torch.Tensor, k0: torch.Tensor,
                  g: Optional[torch.Tensor] = None, ka: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[N, F] = (x - shift[b]) * k1[b] + k0[b], with g and ka: g * ka[b] + that; rows no event owns are 0."""
    dev, x, B = _event_args(x, rowptr, "x", shift, k1, k0, ka)
    N, F = x.shape
    if (g is None) != (ka is None):
        raise ValueError("g and ka are given together or not at all")
    if g is not None:
        g = _f32c(g, "g")
        if g.shape != x.shape or g.device != dev:
            raise ValueError(f"g must be {tuple(x.shape)} on {dev}, got {tuple(g.shape)} on {g.device}")
    out = torch.empty((N, F), dtype=torch.float32, device=dev) if B > 0 else torch.zeros((N, F), dtype=torch.float32, device=dev)
    _t = timer.record('event_affine', dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_event_affine_f32(_ptr(x), _ptr(g), rowptr.data_ptr(), B, N, F, _ptr(shift), _ptr(k1),
                                                     _ptr(k0), _ptr(ka), _ptr(out), _stream(dev)), "dmet_event_affine_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out


# ---- K4 --------------------------------------------------------------------------------------------------------
def met_reduce(w: torch.Tensor, x: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    dev = _require_device(w, x, ptr)
    L = _lib.load()
    w = _f32c(w, "w")
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise TypeError("x must be float32 [N, F>=2] with unit inner stride")
    B = ptr.numel() - 1
    met = torch.empty((B, 2), dtype=torch.float32, device=dev)
    _t = timer.record('met_reduce', dev)
    with _on(dev):
        _lib.check(L.dmet_met_reduce_f32(w.data_ptr(), x.data_ptr(), x.stride(0), ptr.data_ptr(), B, met.data_ptr(),
                                         _stream(dev)), "dmet_met_reduce_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return met


def met_reduce_bwd(g_met: torch.Tensor, x: torch.Tensor, ptr: torch.Tensor,
                   scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g_w[i] = g_met[b,0] * px_i + g_met[b,1] * py_i; scale (optional, one float32 on the device) multiplies g_met first."""
    dev = _require_device(g_met, x, ptr)
    L = _lib.load()
    g_met = _f32c(g_met, "g_met")
    N = x.shape[0]
    B = ptr.numel() - 1
    g_w = torch.empty((N,), dtype=torch.float32, device=dev)
    sp = None
    if scale is not None:
        if scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != dev:
            raise ValueError("met_reduce_bwd: scale must be one float32 on the device")
        sp = scale.data_ptr()
    with _on(dev):
        _lib.check(L.dmet_met_reduce_bwd_scaled_f32(g_met.data_ptr(), sp, x.data_ptr(), x.stride(0), ptr.data_ptr(), B, N,
                                                    g_w.data_ptr(), _stream(dev)), "dmet_met_reduce_bwd_scaled_f32")
    return g_w


def segment_sum_1d(src: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    dev = _require_device(src, ptr)
    L = _lib.load()
    src = _f32c(src, "src")
    B = ptr.numel() - 1
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_segment_sum_1d_f32(src.data_ptr(), ptr.data_ptr(), B, out.data_ptr(), _stream(dev)),
                   "dmet_segment_sum_1d_f32")
    return out


def batch_to_ptr(batch: torch.Tensor, B: int) -> torch.Tensor:
    dev = _require_device(batch)
    L = _lib.load()
    if batch.dtype != torch.int64:
        batch = batch.to(torch.int64)
    batch = batch.contiguous()
    ptr = torch.empty((B + 1,), dtype=torch.int64, device=dev)
    with _on(dev):
        _lib.check(L.dmet_batch_to_ptr(batch.data_ptr(), batch.numel(), B, ptr.data_ptr(), _stream(dev)),
                   "dmet_batch_to_ptr")
    return ptr


# ---- dense-layer weight gradients (N3, first piece) ---------------------------------------------------------------
def xty(A: torch.Tensor, Bm: torch.Tensor) -> torch.Tensor:
    """C[Ha,Hb] = A^T @ B for A[N,Ha], B[N,Hb] (Ha,Hb <= 64), deterministic."""
    dev = _require_device(A, Bm)
    L = _lib.load()
    A = _f32c(A, "A"); Bm = _f32c(Bm, "B")
    N, Ha = A.shape
    Hb = Bm.shape[1]
    C = torch.empty((Ha, Hb), dtype=torch.float32, device=dev)
    _t = timer.record("xty", dev)
    with _on(dev):
        ws = _ws(L.dmet_xty_workspace_bytes(N, Ha, Hb), dev)
        _lib.check(L.dmet_xty_f32(A.data_ptr(), Bm.data_ptr(), N, Ha, Hb, C.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _stream(dev)), "dmet_xty_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return C


def onehot_xty(index: torch.Tensor, Bm: torch.Tensor, num_rows: int) -> torch.Tensor:
    """C[R,Hb] = onehot(index)^T @ B: the weight gradient of an Embedding with R rows."""
    dev = _require_device(index, Bm)
    L = _lib.load()
    if index.dtype != torch.int64:
        raise TypeError("index must be int64")
    index = index.contiguous(); Bm = _f32c(Bm, "B")
    N, Hb = Bm.shape
    C = torch.empty((num_rows, Hb), dtype=torch.float32, device=dev)
    with _on(dev):
        ws = _ws(L.dmet_xty_workspace_bytes(N, num_rows, Hb), dev)
        _lib.check(L.dmet_onehot_xty_f32(index.data_ptr(), Bm.data_ptr(), N, num_rows, Hb, C.data_ptr(), ws.data_ptr(),
                                         ws.numel(), _stream(dev)), "dmet_onehot_xty_f32")
    return C


def _encode_params(params, dev):
    shapes = [(16, 8), (16,), (16, 24), (16,), (32, 32), (32,), (3, 8), (7, 8), (8, 8)]
    if len(params) != 9:
        raise ValueError("encode: expected 9 parameter tensors (Wc, bc, Wk, bk, Wa, ba, Echg, Epdg, Epv)")
    out = []
    for t, shp in zip(params, shapes):
        if tuple(t.shape) != shp:
            raise ValueError(f"encode: parameter of shape {tuple(t.shape)}, expected {shp}")
        if t.device != dev:
            raise ValueError("encode: parameters must be on the device of x")
        out.append(_f32c(t, "param"))
    return out


def _encode_x(x: torch.Tensor, x_cat: torch.Tensor):
    if x.dim() != 2 or x.shape[1] != 8 or x.dtype != torch.float32:
        raise ValueError(f"encode: x_cont must be float32 [N,8], got {tuple(x.shape)} {x.dtype}")
    if x_cat.dim() != 2 or x_cat.shape != (x.shape[0], 3):
        raise ValueError(f"encode: x_cat must be [N,3], got {tuple(x_cat.shape)}")
    if x_cat.dtype == torch.float32:
        # the float columns 8..10 of the same feature matrix (split_features(x, lazy_cat=True)): converted in the kernel
        if (x.stride(1) == 1 and x_cat.stride(1) == 1 and x_cat.stride(0) == x.stride(0) and x.stride(0) >= 11
                and x_cat.data_ptr() == x.data_ptr() + 32):
            return x, None
        x_cat = x_cat.long()
    if x_cat.dtype != torch.int64:
        raise ValueError(f"encode: x_cat must be int64 (or the float columns 8..10 of x), got {x_cat.dtype}")
    return (x if x.stride(1) == 1 else x.contiguous()), x_cat.contiguous()


def encode_fwd(x_cont: torch.Tensor, x_cat: torch.Tensor, params) -> torch.Tensor:
    """h[N,32] = the per-node encoder (graph_met_network.py:48-58 before bn_all) in one kernel."""
    dev = _require_device(x_cont, x_cat)
    L = _lib.load()
    x, xc = _encode_x(x_cont, x_cat)
    ps = _encode_params(params, dev)
    N = x.shape[0]
    h = torch.empty((N, 32), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_encode_fwd_f32(x.data_ptr(), x.stride(0), _ptr(xc), N, *[t.data_ptr() for t in ps],
                                         h.data_ptr(), _stream(dev)), "dmet_encode_fwd_f32")
    return h


def encode_bwd(x_cont: torch.Tensor, x_cat: torch.Tensor, params, h: torch.Tensor, g_h: torch.Tensor):
    """The nine parameter gradients of `encode_fwd` given its output h and dL/dh."""
    dev = _require_device(x_cont, x_cat, h, g_h)
    L = _lib.load()
    x, xc = _encode_x(x_cont, x_cat)
    ps = _encode_params(params, dev)
    h = _f32a(h, "h"); g_h = _f32a(g_h, "g_h")
    N = x.shape[0]
    grads = [torch.empty_like(t) for t in ps]
    if N == 0:
        return [g.zero_() for g in grads]
    with _on(dev):
        ws = _ws(L.dmet_encode_bwd_workspace_bytes(N), dev)
        again = _defer_second_use(dev, *params)
        try:
            _lib.check(L.dmet_encode_bwd_f32(x.data_ptr(), x.stride(0), _ptr(xc), N, *[t.data_ptr() for t in ps],
                                             h.data_ptr(), g_h.data_ptr(), *[g.data_ptr() for g in grads], ws.data_ptr(),
                                             ws.numel(), _stream(dev)), "dmet_encode_bwd_f32")
        finally:
            if again:
                _defer_resume()
        _defer_keep(dev, ws, *grads)
    return grads


def encode_bn_bwd(x_cont: torch.Tensor, x_cat: torch.Tensor, params, h: torch.Tensor, g_y: torch.Tensor,
                  gamma: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor):
    """Backward of bn_all(encode(...)) given dL/d(bn output): (encoder grads [9], g_gamma, g_beta), the BatchNorm's
    backward transform applied inside the encoder's backward kernel (dmet_bn_bwd_stats_f32 + dmet_encode_bn_bwd_f32);
    None when nothing was launched beyond the statistics (the caller keeps the separate steps)."""
    dev = _require_device(x_cont, x_cat, h, g_y)
    L = _lib.load()
    x, xc = _encode_x(x_cont, x_cat)
    ps = _encode_params(params, dev)
    h = _f32c(h, "h"); g_y = _f32c(g_y, "g_y"); gamma = _f32c(gamma.detach(), "gamma")
    N, H = h.shape
    if N == 0 or H != 32:
        return None
    if any(t.data_ptr() % 16 for t in (h, g_y, gamma, mean, invstd)):
        # dmet_encode_bn_bwd_f32 would decline these, and dmet_bn_bwd_stats_f32 before it requires h, g_y, mean and
        # invstd aligned (it would fail the call): the caller's separate steps copy what is unaligned
        return None
    grads = [torch.empty_like(t) for t in ps]
    st = torch.empty((4, H), dtype=torch.float32, device=dev)     # g_gamma, g_beta, mean_g, mean_gx
    fused = ctypes.c_int(0)
    with _on(dev):
        ws = _ws(L.dmet_bn_workspace_bytes(N, H), dev)
        _lib.check(L.dmet_bn_bwd_stats_f32(h.data_ptr(), g_y.data_ptr(), N, H, mean.data_ptr(), invstd.data_ptr(),
                                           st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_bn_bwd_stats_f32")
        ws2 = _ws(L.dmet_encode_bwd_workspace_bytes(N), dev)
        again = _defer_second_use(dev, *params)
        try:
            _lib.check(L.dmet_encode_bn_bwd_f32(x.data_ptr(), x.stride(0), _ptr(xc), N,
                                                *[t.data_ptr() for t in ps], h.data_ptr(), g_y.data_ptr(), gamma.data_ptr(),
                                                mean.data_ptr(), invstd.data_ptr(), st[2].data_ptr(), st[3].data_ptr(),
                                                *[g.data_ptr() for g in grads],
                                                ctypes.cast(ctypes.pointer(fused), ctypes.c_void_p), ws2.data_ptr(), ws2.numel(),
                                                _stream(dev)), "dmet_encode_bn_bwd_f32")
        finally:
            if again:
                _defer_resume()
        if fused.value:
            _defer_keep(dev, ws2, *grads)
        elif not again:     # nothing was launched or queued: the caller's encode_bwd is these parameters' first use
            _DEFER["seen"].difference_update(p.data_ptr() for p in params)
    if not fused.value:
        return None
    return grads, st[0], st[1]


def bn_fwd(x: torch.Tensor, residual: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, eps: float,
           momentum: float, running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], training: bool,
           num_batches_tracked: Optional[torch.Tensor] = None):
    """BatchNorm1d over rows (+ residual): returns (y, save_mean, save_invstd); running stats updated in place, and
    num_batches_tracked (int64 scalar on the device, training mode only) incremented by the statistics kernel."""
    dev = _require_device(x, gamma, beta)
    L = _lib.load()
    x = _f32a(x, "x")
    N, H = x.shape
    if residual is not None:
        residual = _f32a(residual, "residual")
        if residual.shape != x.shape:
            raise ValueError("bn_fwd: residual must have the shape of x")
    for t in (running_mean, running_var):
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float32 or t.numel() != H):
            raise ValueError("bn_fwd: running statistics must be contiguous float32 [H]")
    gamma = _f32a(gamma, "gamma"); beta = _f32a(beta, "beta")
    y = torch.empty_like(x)
    stats = torch.empty((2, H), dtype=torch.float32, device=dev)
    with _on(dev):
        ws = _ws(L.dmet_bn_workspace_bytes(N, H), dev)
        nbt = None
        if num_batches_tracked is not None and training:
            if num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1 or num_batches_tracked.device != dev:
                raise ValueError("bn_fwd: num_batches_tracked must be an int64 scalar on x's device")
            nbt = num_batches_tracked.data_ptr()
        _lib.check(L.dmet_bn_fwd_tracked_f32(x.data_ptr(), _ptr(residual), N, H, gamma.data_ptr(), beta.data_ptr(),
                                             float(eps), float(momentum), _ptr(running_mean), _ptr(running_var), nbt,
                                             1 if training else 0, y.data_ptr(), stats[0].data_ptr(),
                                             stats[1].data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                   "dmet_bn_fwd_tracked_f32")
    return y, stats[0], stats[1]


def bn_stats(x: torch.Tensor, eps: float, momentum: float, running_mean: Optional[torch.Tensor],
             running_var: Optional[torch.Tensor], num_batches_tracked: Optional[torch.Tensor] = None):
    """(save_mean, save_invstd) of the training-mode BatchNorm1d over the rows of x; running statistics and
    num_batches_tracked updated like bn_fwd(training=True).  The transform is applied elsewhere (bn_knn_local_dense)."""
    dev = _require_device(x)
    L = _lib.load()
    x = _f32a(x, "x")
    N, H = x.shape
    stats = torch.empty((2, H), dtype=torch.float32, device=dev)
    with _on(dev):
        ws = _ws(L.dmet_bn_workspace_bytes(N, H), dev)
        _lib.check(L.dmet_bn_stats_f32(x.data_ptr(), N, H, float(eps), float(momentum), _ptr(running_mean),
                                       _ptr(running_var), _ptr(num_batches_tracked),
                                       stats[0].data_ptr(), stats[1].data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                   "dmet_bn_stats_f32")
    return stats[0], stats[1]


def bn_apply(x: torch.Tensor, residual: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
             mean: torch.Tensor, invstd: torch.Tensor) -> torch.Tensor:
    """y = (x - mean) * (gamma * invstd) + beta (+ residual): the transform of bn_fwd with the statistics given
    (bn_stats / bn_eval_stats) -- same kernel, same bits (dmet_bn_apply_f32).  Small vectors that do not start on a
    16-byte boundary (views into somebody else's flat buffer) are copied first."""
    dev = _require_device(x, gamma, beta, mean, invstd)
    L = _lib.load()
    x, residual, vec, aligned = _bn_affine_operands("bn_apply", x, residual, gamma, beta, mean, invstd)
    if not aligned:
        x, vec = _aligned16(x), [_aligned16(v) for v in vec]
        residual = _aligned16(residual) if residual is not None else None
    N, H = x.shape
    y = torch.empty_like(x)
    with _on(dev):
        _lib.check(L.dmet_bn_apply_f32(x.data_ptr(), _ptr(residual), N, H, *[v.data_ptr() for v in vec], y.data_ptr(),
                                       _stream(dev)), "dmet_bn_apply_f32")
    return y


def bn_eval_stats(running_mean: torch.Tensor, running_var: torch.Tensor, eps: float):
    """(mean, invstd) of an eval-mode BatchNorm1d: running_mean and 1 / sqrt(running_var + eps), as bn_fwd(training=False)
    forms them."""
    dev = _require_device(running_mean, running_var)
    L = _lib.load()
    H = running_mean.numel()
    stats = torch.empty((2, H), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_bn_eval_stats_f32(running_mean.data_ptr(), running_var.data_ptr(), H, float(eps),
                                            stats[0].data_ptr(), stats[1].data_ptr(), _stream(dev)), "dmet_bn_eval_stats_f32")
    return stats[0], stats[1]


def bn_knn_local_dense(raw: torch.Tensor, residual: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                       mean: torch.Tensor, invstd: torch.Tensor, ptr: torch.Tensor, k: int, dense=None):
    """y = residual + BatchNorm(raw) (statistics given) fused into the prep launch of the kNN build on y
    (dmet_bn_knn_local_dense_f32).  Returns (y, nbr, dist, loc, pq) -- pq as in knn_local_dense, None without `dense` or
    when the build could not carry the dense layer -- or None when nothing was launched (the build would not take the
    matrix-core path): the caller then applies the transform and builds the graph itself."""
    dev = _require_device(raw, ptr)
    L = _lib.load()
    raw, residual, vec, _ = _bn_affine_operands("bn_knn_local_dense", raw, residual, gamma, beta, mean, invstd)
    N, D = raw.shape
    B = ptr.numel() - 1
    if D != 32 or N == 0 or B == 0 or k > 20:
        return None
    y = torch.empty_like(raw)
    W = b = Pt = Qt = None
    layout, sliced = 0, False
    if dense is not None and tuple(dense[0].shape) == (32, 64):
        W, b, sliced = dense
        W = _f32c(W.detach(), "W")
        b = _f32c(b.detach(), "b") if b is not None else None
        Pt, Qt, layout, sliced = _pq_tables(N, sliced, dev)
    done, fused = ctypes.c_int(0), ctypes.c_int(0)

    def call(nbr, dist, loc_p, ws):     # an unaligned operand goes to the entry as it is: the entry declines
        _lib.check(L.dmet_bn_knn_local_dense_f32(raw.data_ptr(), _ptr(residual), *[v.data_ptr() for v in vec], y.data_ptr(),
                                                 ptr.data_ptr(), B, N, D, k, nbr.data_ptr(), dist.data_ptr(), loc_p, _ptr(W),
                                                 _ptr(b), layout, _ptr(Pt), _ptr(Qt),
                                                 ctypes.cast(ctypes.pointer(done), ctypes.c_void_p),
                                                 ctypes.cast(ctypes.pointer(fused), ctypes.c_void_p), ws.data_ptr(),
                                                 ws.numel(), _stream(dev)), "dmet_bn_knn_local_dense_f32")

    nbr, dist, loc, _, _ = _knn_run(dev, N, k, True, L.dmet_knn_workspace_bytes(N, B, D, k), call)
    if not fused.value:
        return None
    return y, nbr, dist, loc, ((Pt, Qt, sliced) if done.value else None)


def bn_bwd(x: torch.Tensor, g_y: torch.Tensor, gamma: torch.Tensor, save_mean: torch.Tensor, save_invstd: torch.Tensor):
    """(g_x, g_gamma, g_beta) of the training-mode BatchNorm1d."""
    dev = _require_device(x, g_y, gamma)
    L = _lib.load()
    x = _f32a(x, "x"); g_y = _f32a(g_y, "g_y"); gamma = _f32a(gamma, "gamma")
    save_mean = _f32a(save_mean, "save_mean"); save_invstd = _f32a(save_invstd, "save_invstd")
    N, H = x.shape
    g_x = torch.empty_like(x)
    gg = torch.empty((2, H), dtype=torch.float32, device=dev)
    with _on(dev):
        ws = _ws(L.dmet_bn_workspace_bytes(N, H), dev)
        _lib.check(L.dmet_bn_bwd_f32(x.data_ptr(), g_y.data_ptr(), N, H, gamma.data_ptr(), save_mean.data_ptr(),
                                     save_invstd.data_ptr(), g_x.data_ptr(), gg[0].data_ptr(), gg[1].data_ptr(),
                                     ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_bn_bwd_f32")
    return g_x, gg[0], gg[1]


def edgeconv_linear_bwd(x: torch.Tensor, weight: torch.Tensor, g_out: torch.Tensor, arg: Optional[torch.Tensor],
                        gQ: torch.Tensor, want_bias: bool = True, g_add: Optional[torch.Tensor] = None,
                        gq_sliced: bool = False):
    """(gx[N,32], gW[32,64], gb[32] or None) of the fused EdgeConv dense layer (H = 32) from g_out, arg and gQ;
    g_add[N,32] (optional) is added to gx inside the kernel (the residual branch's gradient).  arg: uint8 winning slots
    (255 = none) or uint16 winner ids (0xFFFF = none): g_out is masked to 0 there (R3: such a node produced 0)."""
    dev = _require_device(x, weight, g_out, gQ)
    L = _lib.load()
    weight_key = weight      # the caller's tensor, before any contiguous copy: what tells a second use of the layer
    x = _f32a(x, "x"); weight = _f32c(weight, "weight"); g_out = _f32a(g_out, "g_out"); gQ = _f32a(gQ, "gQ")
    N, H = x.shape
    if H != 32 or tuple(weight.shape) != (32, 64) or g_out.shape != x.shape or (
            tuple(gQ.shape) != ((8, N, 4) if gq_sliced else (N, H))):
        raise ValueError("edgeconv_linear_bwd: built for x[N,32], weight[32,64], gQ[N,32] (or slice-major [8,N,4])")
    if arg is not None and (arg.dtype not in (torch.uint8, torch.uint16, torch.int16) or arg.shape != x.shape
                            or not arg.is_contiguous()):
        raise ValueError("edgeconv_linear_bwd: arg must be contiguous uint8 (slots) or uint16 (winner ids) [N,32]")
    j16 = arg is not None and arg.dtype != torch.uint8
    gx = torch.empty_like(x)
    gW = torch.empty_like(weight)
    gb = torch.empty((H,), dtype=torch.float32, device=dev) if want_bias else None
    with _on(dev):
        ws = _ws(L.dmet_edgeconv_linear_bwd_workspace_bytes(N, H), dev)
        if g_add is not None:
            g_add = _f32a(g_add, "g_add")
            if g_add.shape != x.shape:
                raise ValueError("edgeconv_linear_bwd: g_add must have the shape of x")
        again = _defer_second_use(dev, weight_key)
        try:
            if gq_sliced:
                _lib.check(L.dmet_edgeconv_linear_bwd_sliced_f32(x.data_ptr(), weight.data_ptr(), g_out.data_ptr(),
                                                                 _ptr(arg), int(j16), gQ.data_ptr(), _ptr(g_add), N, H,
                                                                 gx.data_ptr(), gW.data_ptr(), _ptr(gb),
                                                                 ws.data_ptr(), ws.numel(), _stream(dev)),
                           "dmet_edgeconv_linear_bwd_sliced_f32")
            else:
                entry = L.dmet_edgeconv_linear_bwd_add_j16_f32 if j16 else L.dmet_edgeconv_linear_bwd_add_f32
                _lib.check(entry(x.data_ptr(), weight.data_ptr(), g_out.data_ptr(), _ptr(arg), gQ.data_ptr(), _ptr(g_add), N, H,
                                 gx.data_ptr(), gW.data_ptr(), _ptr(gb), ws.data_ptr(), ws.numel(), _stream(dev)),
                           "dmet_edgeconv_linear_bwd_add_j16_f32" if j16 else "dmet_edgeconv_linear_bwd_add_f32")
        finally:
            if again:
                _defer_resume()
        _defer_keep(dev, ws, gW, gb)
    return gx, gW, gb


def gather_max_bwd_lds(g_out: torch.Tensor, arg: torch.Tensor, nbr: torch.Tensor, ptr: torch.Tensor,
                       nbr_local: Optional[torch.Tensor] = None, max_nodes: Optional[int] = None,
                       sliced: bool = False) -> torch.Tensor:
    """gQ[N,32] by per-event LDS scatter with exact integer sums (no reverse index); see include/dmet.h.
    max_nodes: the batch's largest event when the caller knows it (a hint: workgroups sized for small events).
    sliced: gQ comes back slice-major, [8, N, 4] (for edgeconv_linear_bwd(..., gq_sliced=True))."""
    dev = _require_device(g_out, arg, nbr, ptr)
    g_out = _f32a(g_out, "g_out")
    N, H = g_out.shape
    if arg.dtype != torch.uint8 or not arg.is_contiguous() or nbr.dtype != torch.int32 or not nbr.is_contiguous():
        raise TypeError("gather_max_bwd_lds: arg must be contiguous uint8, nbr contiguous int32")
    _check_nbr_local(nbr_local, nbr)
    sliced = bool(sliced and H == 32)
    gQ = torch.empty((8, N, 4) if sliced else (N, H), dtype=torch.float32, device=dev)
    _gather_run(dev, 'gather_max_bwd', None, "dmet_gather_max_bwd_sliced_f32" if sliced else "dmet_gather_max_bwd_lds16_cap_f32",
                g_out.data_ptr(), arg.data_ptr(), nbr.data_ptr(), _ptr(nbr_local),
                ptr.data_ptr(), ptr.numel() - 1, N, nbr.shape[1], H, gQ.data_ptr(), int(max_nodes or 0))
    return gQ


def met_loss(met: torch.Tensor, truth: torch.Tensor):
    """(loss[1], d loss / d met [B,2]) of 0.5 * mean((met + truth)^2 summed over px, py)."""
    dev = _require_device(met, truth)
    L = _lib.load()
    met = _f32c(met, "met"); truth = _f32c(truth, "truth")
    if met.dim() != 2 or met.shape[1] != 2 or truth.shape[0] != met.shape[0] or truth.shape[1] < 2:
        raise ValueError("met_loss: met must be [B,2], truth [B,>=2]")
    B = met.shape[0]
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    g = torch.empty_like(met)
    with _on(dev):    # px, py are columns 0, 1 of the rows: no [B,2] copy of the [B,11] target
        _lib.check(L.dmet_met_loss_strided_f32(met.data_ptr(), truth.data_ptr(), truth.stride(0), B, loss.data_ptr(),
                                               g.data_ptr(), _stream(dev)), "dmet_met_loss_strided_f32")
    return loss, g


def _head_params(params, dev):
    shapes = [(16, 32), (16,), (1, 16), (1,)]
    if len(params) != 4:
        raise ValueError("head: expected (W1, b1, W2, b2)")
    out = []
    for t, shp in zip(params, shapes):
        if tuple(t.shape) != shp or t.device != dev:
            raise ValueError(f"head: parameter of shape {tuple(t.shape)}, expected {shp} on the device of emb")
        out.append(_f32c(t, "param"))
    return out


def head_fwd(emb: torch.Tensor, params) -> torch.Tensor:
    """sigmoid(W2 . ELU(W1 . emb + b1) + b2) per node: [N] from emb[N,32]."""
    dev = _require_device(emb)
    L = _lib.load()
    emb = _f32a(emb, "emb")
    if emb.dim() != 2 or emb.shape[1] != 32:
        raise ValueError("head: emb must be [N,32]")
    ps = _head_params(params, dev)
    N = emb.shape[0]
    out = torch.empty((N,), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_head_fwd_f32(emb.data_ptr(), N, *[t.data_ptr() for t in ps], out.data_ptr(), _stream(dev)),
                   "dmet_head_fwd_f32")
    return out


def bn_head_fwd(raw: torch.Tensor, residual: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                mean: torch.Tensor, invstd: torch.Tensor, params):
    """(emb, out): emb = residual + BatchNorm(raw) (statistics given) formed inside the head's forward launch and out =
    head_fwd(emb, params) (dmet_bn_head_fwd_f32); None when nothing was launched (the caller keeps the two steps)."""
    dev = _require_device(raw)
    L = _lib.load()
    if raw.dim() != 2 or raw.shape[1] != 32:
        return None
    raw, residual, vec, _ = _bn_affine_operands("bn_head_fwd", raw, residual, gamma, beta, mean, invstd)
    ps = _head_params(params, dev)
    N = raw.shape[0]
    emb = torch.empty_like(raw)
    out = torch.empty((N,), dtype=torch.float32, device=dev)
    fused = ctypes.c_int(0)
    with _on(dev):   # an unaligned operand goes to the entry as it is: the entry declines
        _lib.check(L.dmet_bn_head_fwd_f32(raw.data_ptr(), _ptr(residual), *[v.data_ptr() for v in vec], emb.data_ptr(), N,
                                          *[t.data_ptr() for t in ps], out.data_ptr(),
                                          ctypes.cast(ctypes.pointer(fused), ctypes.c_void_p), _stream(dev)),
                   "dmet_bn_head_fwd_f32")
    return (emb, out) if fused.value else None


def head_bwd(emb: torch.Tensor, params, out: torch.Tensor, g_out: torch.Tensor):
    """(g_emb, gW1, gb1, gW2, gb2) of head_fwd."""
    dev = _require_device(emb, out, g_out)
    L = _lib.load()
    # emb rows are read as float4 (copied when unaligned); out and g_out are read one element per node: any 4-byte place
    emb = _f32a(emb, "emb"); out = _f32c(out, "out"); g_out = _f32c(g_out, "g_out")
    ps = _head_params(params, dev)
    N = emb.shape[0]
    g_emb = torch.empty_like(emb)
    grads = [torch.empty_like(t) for t in ps]
    if N == 0:
        return [g_emb] + [g.zero_() for g in grads]
    with _on(dev):
        ws = _ws(L.dmet_head_bwd_workspace_bytes(N), dev)
        again = _defer_second_use(dev, *params)
        try:
            _lib.check(L.dmet_head_bwd_f32(emb.data_ptr(), N, ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr(),
                                           out.data_ptr(), g_out.data_ptr(), g_emb.data_ptr(),
                                           *[g.data_ptr() for g in grads], ws.data_ptr(), ws.numel(), _stream(dev)),
                       "dmet_head_bwd_f32")
        finally:
            if again:
                _defer_resume()
        _defer_keep(dev, ws, *grads)
    return [g_emb] + grads


def table_rowptr(nbr: torch.Tensor, cnt: Optional[torch.Tensor]) -> torch.Tensor:
    """rowptr[N+1] int32: exclusive prefix sum of the number of valid entries per row of a neighbour table."""
    dev = _require_device(nbr)
    L = _lib.load()
    N, k = nbr.shape
    rowptr = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    if N:
        deg = torch.empty((N,), dtype=torch.int32, device=dev)
        with _on(dev):
            _lib.check(L.dmet_table_degree(nbr.data_ptr(), _ptr(cnt), N, k,
                                           deg.data_ptr(), _stream(dev)), "dmet_table_degree")
        torch.cumsum(deg, 0, dtype=torch.int32, out=rowptr[1:])
    return rowptr


def table_edges(nbr: torch.Tensor, cnt: Optional[torch.Tensor], rowptr: torch.Tensor, num_edges: int, swap: bool,
                want_index64: bool, want_int32: bool):
    """(edge_index [2,E] int64 or None, src32 [E] or None, tgt32 [E] or None) of a neighbour table."""
    dev = _require_device(nbr, rowptr)
    L = _lib.load()
    N, k = nbr.shape
    ei = torch.empty((2, num_edges), dtype=torch.int64, device=dev) if want_index64 else None
    s32 = torch.empty((num_edges,), dtype=torch.int32, device=dev) if want_int32 else None
    t32 = torch.empty((num_edges,), dtype=torch.int32, device=dev) if want_int32 else None
    if N and num_edges:
        with _on(dev):
            _lib.check(L.dmet_table_edges(nbr.data_ptr(), _ptr(cnt), rowptr.data_ptr(), N, k, 1 if swap else 0,
                                          ei[0].data_ptr() if ei is not None else None,
                                          ei[1].data_ptr() if ei is not None else None,
                                          _ptr(s32), _ptr(t32), _stream(dev)), "dmet_table_edges")
    return ei, s32, t32


# ---- graph coarsening (csrc/pool.hip): graclus, normalized cut, pair pooling ------------------------------------------
def graclus(rowptr: torch.Tensor, col: torch.Tensor, weight: Optional[torch.Tensor], ptr: torch.Tensor, seed: int,
            max_rounds: int = 0, want_rounds: bool = False):
    """(cluster[N] int64, partner[N] int32, rounds[B] int32 or None) of dmet_graclus_f32."""
    dev = _require_device(rowptr, col, weight, ptr)
    L = _lib.load()
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or ptr.dtype != torch.int64:
        raise TypeError("graclus: rowptr / ptr must be int64 and col int32")
    N = rowptr.numel() - 1
    B = ptr.numel() - 1
    if weight is not None:
        weight = _f32c(weight, "weight")
    cluster = torch.empty((N,), dtype=torch.int64, device=dev)
    partner = torch.empty((N,), dtype=torch.int32, device=dev)
    rounds = torch.empty((max(B, 1),), dtype=torch.int32, device=dev) if want_rounds else None
    _t = timer.record('graclus', dev)
    with _on(dev):
        ws = _ws(L.dmet_graclus_workspace_bytes(N), dev)
        _lib.check(L.dmet_graclus_f32(rowptr.data_ptr(), col.data_ptr(), _ptr(weight),
                                      ptr.data_ptr(), B, N, int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_rounds),
                                      cluster.data_ptr(), partner.data_ptr(),
                                      _ptr(rounds), ws.data_ptr(), ws.numel(),
                                      _stream(dev)), "dmet_graclus_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return cluster, partner, (rounds[:B] if rounds is not None else None)


def normalized_cut(edge_index: torch.Tensor, N: int, attr: Optional[torch.Tensor] = None,
                   x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w[E] of dmet_normalized_cut_f32 (attr[E]) or dmet_normalized_cut_2d_f32 (x[N,D])."""
    dev = _require_device(edge_index, attr, x)
    L = _lib.load()
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise TypeError("edge_index must be an int64 [2, E] tensor")
    ei = edge_index.contiguous()
    E = ei.shape[1]
    w = torch.empty((E,), dtype=torch.float32, device=dev)
    row, col = ei[0], ei[1]
    _t = timer.record('normalized_cut', dev)
    with _on(dev):
        ws = _ws(L.dmet_normalized_cut_workspace_bytes(N), dev)
        if x is not None:
            x = _f32c(x, "x")
            _lib.check(L.dmet_normalized_cut_2d_f32(row.data_ptr(), col.data_ptr(), E, N, x.data_ptr(), x.shape[1],
                                                    w.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                       "dmet_normalized_cut_2d_f32")
        else:
            attr = _f32c(attr.reshape(-1), "edge_attr")
            if attr.numel() != E:
                raise ValueError(f"edge_attr must hold one value per edge ({E}), got {attr.numel()}")
            _lib.check(L.dmet_normalized_cut_f32(row.data_ptr(), col.data_ptr(), E, N, attr.data_ptr(), w.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_normalized_cut_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return w


def pool_pairs_index(partner: torch.Tensor, ptr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cid[N] int64, pooled_ptr[B+1] int64) of dmet_pool_pairs_index."""
    dev = _require_device(partner, ptr)
    L = _lib.load()
    N = partner.numel()
    B = ptr.numel() - 1
    cid = torch.empty((N,), dtype=torch.int64, device=dev)
    pooled_ptr = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    _t = timer.record('pool_pairs_index', dev)
    with _on(dev):
        ws = _ws(L.dmet_pool_pairs_workspace_bytes(N, B), dev)
        _lib.check(L.dmet_pool_pairs_index(partner.data_ptr(), ptr.data_ptr(), B, N, cid.data_ptr(), pooled_ptr.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_pool_pairs_index")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return cid, pooled_ptr


def pool_pairs(x: torch.Tensor, partner: torch.Tensor, cid: torch.Tensor, ptr: Optional[torch.Tensor], C: int,
               want_max: bool, want_mean: bool, want_batch: bool):
    """(out_max, arg, out_mean, pooled_batch) of dmet_pool_pairs_f32; the ones not asked for are None."""
    dev = _require_device(x, partner, cid, ptr)
    L = _lib.load()
    x = _f32c(x, "x")
    N, F = x.shape
    B = ptr.numel() - 1 if ptr is not None else 0
    out_max = torch.empty((C, F), dtype=torch.float32, device=dev) if want_max else None
    arg = torch.empty((C, F), dtype=torch.int32, device=dev) if want_max else None
    out_mean = torch.empty((C, F), dtype=torch.float32, device=dev) if want_mean else None
    pb = torch.empty((C,), dtype=torch.int64, device=dev) if want_batch else None
    _t = timer.record('pool_pairs', dev)
    with _on(dev):
        _lib.check(L.dmet_pool_pairs_f32(x.data_ptr(), N, F, partner.data_ptr(), cid.data_ptr(), _ptr(ptr), B, C,
                                         _ptr(out_max), _ptr(arg), _ptr(out_mean), _ptr(pb), _stream(dev)), "dmet_pool_pairs_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out_max, arg, out_mean, pb


def pool_pairs_bwd(g_max: Optional[torch.Tensor], arg: Optional[torch.Tensor], g_mean: Optional[torch.Tensor],
                   partner: torch.Tensor, cid: torch.Tensor, F: int, C: int) -> torch.Tensor:
    dev = _require_device(g_max, arg, g_mean, partner, cid)
    L = _lib.load()
    N = partner.numel()
    g_max = _f32c(g_max, "g_max") if g_max is not None else None
    g_mean = _f32c(g_mean, "g_mean") if g_mean is not None else None
    gx = torch.empty((N, F), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.dmet_pool_pairs_bwd_f32(_ptr(g_max), _ptr(arg), _ptr(g_mean), partner.data_ptr(), cid.data_ptr(), N, F, C,
                                             gx.data_ptr(), _stream(dev)), "dmet_pool_pairs_bwd_f32")
    return gx


# ---- farthest point sampling (csrc/fps.hip) -----------------------------------------------------------------------------
FPS_THREADS = 1024          # DMET_FPS_THREADS: the workgroup of an event
FPS_LDS_FLOATS = 36864      # DMET_FPS_LDS_FLOATS


def FPS_LDS_NODES(D: int) -> int:
    """DMET_FPS_LDS_NODES(D): the largest event whose D coordinates and running distances stay in LDS."""
    return FPS_LDS_FLOATS // (int(D) + 1)


def fps(x: torch.Tensor, ptr: torch.Tensor, out_ptr: torch.Tensor, start: Optional[torch.Tensor], M: int) -> torch.Tensor:
    """out[M] int64 of dmet_fps_f32: event b's out_ptr[b+1] - out_ptr[b] picks as global node ids.  start: int64 [B]
    event-local first picks, or None (node 0 of every event).  M: out_ptr[B] as the caller knows it."""
    dev = _require_device(x, ptr, out_ptr, start)
    L = _lib.load()
    x = _f32c(x.detach(), "x")
    if x.dim() != 2:
        raise ValueError(f"x must be [N, D], got {tuple(x.shape)}")
    if ptr.dtype != torch.int64 or out_ptr.dtype != torch.int64 or ptr.numel() != out_ptr.numel() or ptr.numel() < 1:
        raise TypeError("fps: ptr and out_ptr must be int64 vectors over the same events")
    if start is not None and (start.dtype != torch.int64 or start.numel() != ptr.numel() - 1):
        raise TypeError("fps: start must be an int64 vector with one entry per event")
    N, D = x.shape
    B = ptr.numel() - 1
    ptr, out_ptr = ptr.contiguous(), out_ptr.contiguous()
    start = start.contiguous() if start is not None else None
    out = torch.empty((int(M),), dtype=torch.int64, device=dev)
    _t = timer.record('fps', dev)
    with _on(dev):
        ws = _ws(L.dmet_fps_workspace_bytes(N, B, D), dev)
        _lib.check(L.dmet_fps_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, out_ptr.data_ptr(),
                                  _ptr(start), int(M), out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _stream(dev)), "dmet_fps_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out


# ---- selection pooling (csrc/select.hip) --------------------------------------------------------------------------------
SELECT_LDS_NODES = 16384    # DMET_SELECT_LDS_NODES: the largest event whose keys are sorted in LDS
SELECT_MAX_K = 1024         # DMET_SELECT_MAX_K


def _sel_vec(t: torch.Tensor, name: str, dtype: torch.dtype, n: Optional[int] = None) -> torch.Tensor:
    if t.dtype != dtype or t.dim() != 1 or (n is not None and t.numel() != n):
        raise TypeError(f"{name} must be a 1-D {dtype} tensor" + (f" of {n} entries" if n is not None else "") +
                        f", got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _topk(score: torch.Tensor, ptr: torch.Tensor, out_ptr: torch.Tensor, M: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(perm[M] int64, node_map[N] int32) of dmet_topk_f32: event b's best min(r_b, n_b) nodes by descending canonical
    score (ties to the lower index) in its slots out_ptr[b] .. out_ptr[b+1], -1 in the slots left; node_map[i] = the
    position of node i in perm or -1.  M: the size of perm as the caller knows it."""
    dev = _require_device(score, ptr, out_ptr)
    L = _lib.load()
    score = _f32c(score.detach(), "score")
    if score.dim() != 1:
        raise ValueError(f"score must be [N], got {tuple(score.shape)}")
    ptr = _sel_vec(ptr, "ptr", torch.int64)
    out_ptr = _sel_vec(out_ptr, "out_ptr", torch.int64, ptr.numel())
    if ptr.numel() < 1:
        raise TypeError("topk: ptr and out_ptr must hold B + 1 entries")
    N, B = score.numel(), ptr.numel() - 1
    perm = torch.empty((int(M),), dtype=torch.int64, device=dev)
    node_map = torch.empty((N,), dtype=torch.int32, device=dev) if B > 0 else torch.full((N,), -1, dtype=torch.int32, device=dev)
    if B == 0 and M:
        perm.fill_(-1)
    _t = timer.record('topk', dev)
    with _on(dev):
        ws = _ws(L.dmet_topk_workspace_bytes(N), dev)
        _lib.check(L.dmet_topk_f32(_ptr(score), ptr.data_ptr(), B, N, out_ptr.data_ptr(), int(M), _ptr(perm), _ptr(node_map),
                                   ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_topk_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return perm, node_map


def _select_rows(x: torch.Tensor, s: Optional[torch.Tensor], perm: torch.Tensor) -> torch.Tensor:
    """out[M, F] = x[perm] * s[perm][:, None] (s None: x[perm]); rows with perm < 0 are zeros (dmet_select_rows_f32)."""
    dev = _require_device(x, s, perm)
    x = _f32c(x.detach(), "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"x must be [N, F] with F >= 1, got {tuple(x.shape)}")
    N, F = x.shape
    s = _sel_vec(_f32c(s.detach(), "s"), "s", torch.float32, N) if s is not None else None
    perm = _sel_vec(perm, "perm", torch.int64)
    M = perm.numel()
    out = torch.empty((M, F), dtype=torch.float32, device=dev)
    _t = timer.record('select_rows', dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_select_rows_f32(_ptr(x), s.data_ptr() if s is not None and N else None, _ptr(perm), N, M, F,
                                                    _ptr(out), _stream(dev)), "dmet_select_rows_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out


def _select_rows_bwd(g: torch.Tensor, x: Optional[torch.Tensor], s: Optional[torch.Tensor], node_map: torch.Tensor,
                    need_gx: bool = True, need_gs: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(gx[N, F] or None, gs[N] or None) of dmet_select_rows_bwd_f32 for g[M, F]; x is needed for gs only."""
    dev = _require_device(g, x, s, node_map)
    g = _f32c(g.detach(), "g")
    if g.dim() != 2 or g.shape[1] < 1:
        raise ValueError(f"g must be [M, F] with F >= 1, got {tuple(g.shape)}")
    M, F = g.shape
    node_map = _sel_vec(node_map, "node_map", torch.int32)
    N = node_map.numel()
    if need_gs:
        if x is None:
            raise ValueError("select_rows_bwd: gs needs x")
        x = _f32c(x.detach(), "x")
        if tuple(x.shape) != (N, F):
            raise ValueError(f"x must be [{N}, {F}], got {tuple(x.shape)}")
    s = _sel_vec(_f32c(s.detach(), "s"), "s", torch.float32, N) if s is not None else None
    gx = torch.empty((N, F), dtype=torch.float32, device=dev) if need_gx else None
    gs = torch.empty((N,), dtype=torch.float32, device=dev) if need_gs else None
    _t = timer.record('select_rows_bwd', dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_select_rows_bwd_f32(_ptr(g), _ptr(x) if need_gs else None,
                                                        s.data_ptr() if s is not None and N else None, _ptr(node_map), N, M, F,
                                                        _ptr(gx), _ptr(gs), _stream(dev)), "dmet_select_rows_bwd_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return gx, gs


def _filter_table(nbr: torch.Tensor, cnt: Optional[torch.Tensor], perm: torch.Tensor,
                 node_map: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out_nbr[M, k] int32, out_cnt[M] int32) of dmet_filter_table: row perm[r] of nbr, its picked entries relabelled
    through node_map and packed to the left, -1 behind them."""
    dev = _require_device(nbr, cnt, perm, node_map)
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or not 1 <= nbr.shape[1] <= SELECT_MAX_K:
        raise ValueError(f"nbr must be int32 [N, k] with 1 <= k <= {SELECT_MAX_K}, got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    N, k = nbr.shape
    cnt = _sel_vec(cnt, "cnt", torch.int32, N) if cnt is not None else None
    perm = _sel_vec(perm, "perm", torch.int64)
    node_map = _sel_vec(node_map, "node_map", torch.int32, N)
    M = perm.numel()
    out_nbr = torch.empty((M, k), dtype=torch.int32, device=dev)
    out_cnt = torch.empty((M,), dtype=torch.int32, device=dev)
    _t = timer.record('filter_table', dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_filter_table(_ptr(nbr), _ptr(cnt), _ptr(perm), _ptr(node_map), N, M, k, _ptr(out_nbr),
                                                 _ptr(out_cnt), _stream(dev)), "dmet_filter_table")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out_nbr, out_cnt


def _filter_edges(edge_index: torch.Tensor, node_map: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(edge_index'[2, E'] int64, kept[E'] int64, nbad int32 [1]) of dmet_filter_edges_count / _write: the edges whose ends
    are both picked, relabelled through node_map, in the caller's order; kept = their positions in edge_index; nbad = the
    number of edges with an end outside [0, N) (dropped; left on the device for a deferred check).  One host read: E'."""
    dev = _require_device(edge_index, node_map)
    L = _lib.load()
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    if edge_index.dtype != torch.int64:
        raise TypeError(f"edge_index must be int64 (torch.long), got {edge_index.dtype}")
    node_map = _sel_vec(node_map, "node_map", torch.int32)
    edge_index = edge_index.contiguous()
    E, N = edge_index.shape[1], node_map.numel()
    if E == 0:
        return (torch.zeros((2, 0), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev),
                torch.zeros((1,), dtype=torch.int32, device=dev))
    row, col = edge_index[0], edge_index[1]
    total = torch.empty((1,), dtype=torch.int64, device=dev)
    nbad = torch.empty((1,), dtype=torch.int32, device=dev)
    _t = timer.record('filter_edges', dev)
    with _on(dev):
        ws = _ws(L.dmet_filter_edges_workspace_bytes(E), dev)
        _lib.check(L.dmet_filter_edges_count(row.data_ptr(), col.data_ptr(), E, _ptr(node_map), N, total.data_ptr(),
                                             nbad.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                   "dmet_filter_edges_count")
        Eout = int(total.item())
        out = torch.empty((2, Eout), dtype=torch.int64, device=dev)
        kept = torch.empty((Eout,), dtype=torch.int64, device=dev)
        _lib.check(L.dmet_filter_edges_write(row.data_ptr(), col.data_ptr(), E, _ptr(node_map), N, ws.data_ptr(), ws.numel(),
                                             Eout, _ptr(out), _ptr(kept), _stream(dev)), "dmet_filter_edges_write")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return out, kept, nbad


# ---- voxel clustering (csrc/voxel.hip) -----------------------------------------------------------------------------------
VOXEL_MAX_DIM = 8           # DMET_VOXEL_MAX_DIM


def _voxel_cells(pos: torch.Tensor, grid: torch.Tensor, ptr: torch.Tensor,
                 batch: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(id[N] int64, cell[N] int32 holding the uint32 event-local cell ids, nvox[D + 1] int64, flags[2] int32) of
    dmet_voxel_cells_f32 for pos[N, D] fp32 and grid[3, D] fp32 = (size, start, end) on the device.  flags[0]: the cell
    count of an event passed 2^32 - 1 and was cut; flags[1]: batch disagrees with ptr."""
    dev = _require_device(pos, grid, ptr, batch)
    pos = _f32c(pos.detach(), "pos")
    if pos.dim() != 2 or not 1 <= pos.shape[1] <= VOXEL_MAX_DIM:
        raise ValueError(f"pos must be [N, D] with 1 <= D <= {VOXEL_MAX_DIM}, got {tuple(pos.shape)}")
    N, D = pos.shape
    grid = _f32c(grid, "grid")
    if tuple(grid.shape) != (3, D):
        raise ValueError(f"grid must be [3, {D}], got {tuple(grid.shape)}")
    ptr = _sel_vec(ptr, "ptr", torch.int64)
    B = ptr.numel() - 1
    batch = _sel_vec(batch, "batch", torch.int64, N) if batch is not None else None
    ids = torch.empty((N,), dtype=torch.int64, device=dev)
    cell = torch.empty((N,), dtype=torch.int32, device=dev)
    nvox = torch.empty((D + 1,), dtype=torch.int64, device=dev)
    flags = torch.empty((2,), dtype=torch.int32, device=dev)
    _t = timer.record('voxel_cells', dev)
    with _on(dev):
        _lib.check(_lib.load().dmet_voxel_cells_f32(_ptr(pos), N, D, grid.data_ptr(), ptr.data_ptr(), B, _ptr(batch),
                                                    nvox.data_ptr(), flags.data_ptr(), _ptr(ids), _ptr(cell), _stream(dev)),
                   "dmet_voxel_cells_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return ids, cell, nvox, flags


def _voxel_coarsen(cell: torch.Tensor, ptr: torch.Tensor):
    """(node_map[N] int64, order[N] int64, rowptr[N + 1] int32, batch[N] int64, ptr[B + 1] int64, record[3] int64) of
    dmet_voxel_coarsen for the event-local cell ids of _voxel_cells, N > 0.  rowptr and batch are written up to C + 1 and
    C entries, C = record[0] (left on the device: the caller reads the record and cuts them)."""
    dev = _require_device(cell, ptr)
    L = _lib.load()
    cell = _sel_vec(cell, "cell", torch.int32)
    ptr = _sel_vec(ptr, "ptr", torch.int64)
    N, B = cell.numel(), ptr.numel() - 1
    if N < 1 or B < 1:
        raise ValueError(f"voxel_coarsen: needs nodes and events, got N={N}, B={B}")
    node_map = torch.empty((N,), dtype=torch.int64, device=dev)
    order = torch.empty((N,), dtype=torch.int64, device=dev)
    rowptr = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    out_batch = torch.empty((N,), dtype=torch.int64, device=dev)
    out_ptr = torch.empty((B + 1,), dtype=torch.int64, device=dev)
    record = torch.empty((3,), dtype=torch.int64, device=dev)
    _t = timer.record('voxel_coarsen', dev)
    with _on(dev):
        ws = _ws(L.dmet_voxel_coarsen_workspace_bytes(N, B), dev)
        _lib.check(L.dmet_voxel_coarsen(cell.data_ptr(), ptr.data_ptr(), B, N, node_map.data_ptr(), order.data_ptr(),
                                        rowptr.data_ptr(), out_batch.data_ptr(), out_ptr.data_ptr(), record.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_voxel_coarsen")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return node_map, order, rowptr, out_batch, out_ptr, record


# ---- edge pooling (csrc/edge_match.hip) ------------------------------------------------------------------------------------
EDGE_MATCH_LDS_NODES = 16384    # DMET_EDGE_MATCH_LDS_NODES: the largest event whose state words stay in LDS


def _edge_match(rowptr: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor, perm: Optional[torch.Tensor],
                score: torch.Tensor, ptr: torch.Tensor, want_rounds: bool = False):
    """(cluster[N] int64, partner[N] int32, edge[N] int64, rounds[B] int32 or None, flags[3] int32) of dmet_edge_match_f32
    for edges grouped by target (rowptr[N + 1], src[E], tgt[E] int32), perm[E] int32 = the caller-order id of every
    grouped position (None: the position), score[E] by grouped position.  flags: an end outside [0, N) | an edge across
    two events | the round bound was reached."""
    dev = _require_device(rowptr, src, tgt, perm, score, ptr)
    L = _lib.load()
    rowptr = _sel_vec(rowptr, "rowptr", torch.int32)
    if rowptr.numel() < 1:
        raise TypeError("edge_match: rowptr must hold N + 1 entries")
    N = rowptr.numel() - 1
    src = _sel_vec(src, "src", torch.int32)
    E = src.numel()
    tgt = _sel_vec(tgt, "tgt", torch.int32, E)
    perm = _sel_vec(perm, "perm", torch.int32, E) if perm is not None else None
    score = _sel_vec(_f32c(score.detach(), "score"), "score", torch.float32, E)
    ptr = _sel_vec(ptr, "ptr", torch.int64)
    if ptr.numel() < 1:
        raise TypeError("edge_match: ptr must hold B + 1 entries")
    B = ptr.numel() - 1
    if B > 0 and N > 0:
        cluster = torch.empty((N,), dtype=torch.int64, device=dev)
        partner = torch.empty((N,), dtype=torch.int32, device=dev)
        edge = torch.empty((N,), dtype=torch.int64, device=dev)
    else:       # no event owns a node: the kernel is not launched
        cluster = torch.arange(N, dtype=torch.int64, device=dev)
        partner = torch.full((N,), -1, dtype=torch.int32, device=dev)
        edge = torch.full((N,), -1, dtype=torch.int64, device=dev)
    rounds = torch.empty((B,), dtype=torch.int32, device=dev) if want_rounds else None
    flags = torch.empty((3,), dtype=torch.int32, device=dev)
    _t = timer.record('edge_match', dev)
    with _on(dev):
        ws = _ws(L.dmet_edge_match_workspace_bytes(N, E), dev)
        _lib.check(L.dmet_edge_match_f32(rowptr.data_ptr(), _ptr(src), _ptr(tgt), _ptr(perm), _ptr(score), E, ptr.data_ptr(), B, N,
                                         _ptr(cluster), _ptr(partner), _ptr(edge), _ptr(rounds), flags.data_ptr(), _ptr(ws),
                                         ws.numel(), _stream(dev)), "dmet_edge_match_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return cluster, partner, edge, rounds, flags


# ---- connected components and DBSCAN (csrc/components.hip) ---------------------------------------------------------------
COMPONENTS_LDS_NODES = 16384    # DMET_COMPONENTS_LDS_NODES: the largest event whose parent words stay in LDS
COMPONENTS_CC, COMPONENTS_DBSCAN = 0, 1


def _mask_u8(t: Optional[torch.Tensor], name: str, n: int) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.bool or t.numel() != n:
        raise TypeError(f"{name} must be a bool tensor of {n} values, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous().view(torch.uint8).view(-1)


def _components(ptr: torch.Tensor, N: int, *, nbr: Optional[torch.Tensor] = None, cnt: Optional[torch.Tensor] = None,
                rowptr: Optional[torch.Tensor] = None, src: Optional[torch.Tensor] = None,
                tgt: Optional[torch.Tensor] = None, edge_mask: Optional[torch.Tensor] = None,
                node_mask: Optional[torch.Tensor] = None, min_samples: Optional[int] = None, count_self: bool = False,
                lds_nodes: int = 0):
    """(labels[N] int64, core[N] bool or None, nclusters[B] int64 or None, flags[4] int32) of dmet_components_i32 for a
    table (nbr[N, k] int32, cnt[N] int32 or None) or a by-target list (rowptr[N + 1], src[E], tgt[E] int32).
    min_samples=None: connected components, labels = the smallest global id of every component (edge_mask / node_mask:
    bool, one value per position / node); else DBSCAN mode: event-local cluster numbers, the core mask and the cluster
    count of every event.  flags: entries with an end outside [0, N) | entries across two events | a loop bound was
    reached | (DBSCAN, table) rows that fill every slot.  lds_nodes: the largest event kept in LDS (0: the default)."""
    dev = _require_device(ptr, nbr, cnt, rowptr, src, tgt, edge_mask, node_mask)
    L = _lib.load()
    N = int(N)
    ptr = _sel_vec(ptr, "ptr", torch.int64)
    if ptr.numel() < 1:
        raise TypeError("components: ptr must hold B + 1 entries")
    B = ptr.numel() - 1
    if (nbr is None) == (rowptr is None):
        raise TypeError("components: pass a table (nbr) or a grouped list (rowptr, src, tgt), one of them")
    k, E = 0, 0
    if nbr is not None:
        if nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != N:
            raise TypeError(f"components: nbr must be an int32 [{N}, k] tensor, got {nbr.dtype} {tuple(nbr.shape)}")
        nbr = nbr.contiguous()
        k = nbr.shape[1]
        cnt = _sel_vec(cnt, "cnt", torch.int32, N) if cnt is not None else None
        positions = N * k
    else:
        rowptr = _sel_vec(rowptr, "rowptr", torch.int32, N + 1)
        src = _sel_vec(src, "src", torch.int32)
        E = src.numel()
        tgt = _sel_vec(tgt, "tgt", torch.int32, E)
        positions = E
    dbscan = min_samples is not None
    if dbscan and (edge_mask is not None or node_mask is not None):
        raise TypeError("components: DBSCAN mode takes no masks")
    edge_mask = _mask_u8(edge_mask, "edge_mask", positions)
    node_mask = _mask_u8(node_mask, "node_mask", N)
    labels = torch.empty((N,), dtype=torch.int64, device=dev)
    core = torch.empty((N,), dtype=torch.bool, device=dev) if dbscan else None
    nclusters = torch.empty((B,), dtype=torch.int64, device=dev) if dbscan else None
    flags = torch.empty((4,), dtype=torch.int32, device=dev)
    _t = timer.record('components', dev)
    with _on(dev):
        ws = _ws(L.dmet_components_workspace_bytes(N), dev)
        _lib.check(L.dmet_components_i32(_ptr(nbr), k, _ptr(cnt), rowptr.data_ptr() if rowptr is not None else None, _ptr(src),
                                         _ptr(tgt), E, _ptr(edge_mask), _ptr(node_mask), ptr.data_ptr(), B, N,
                                         COMPONENTS_DBSCAN if dbscan else COMPONENTS_CC, int(min_samples) if dbscan else 0,
                                         1 if count_self else 0, _ptr(labels), _ptr(core), _ptr(nclusters), flags.data_ptr(),
                                         int(lds_nodes), ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_components_i32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return labels, core, nclusters, flags


# ---------------------------------------------------------------------------------------------------------------
# Condensation clustering (csrc/condense.hip)
# ---------------------------------------------------------------------------------------------------------------
CONDENSE_LDS_NODES = 16384      # DMET_CONDENSE_LDS_NODES: the largest event whose state words stay in LDS
CONDENSE_WINDOW = 64            # DMET_CONDENSE_WINDOW
CONDENSE_MAX_DIM = 8            # DMET_CONDENSE_MAX_DIM


def _condense(beta: torch.Tensor, x: torch.Tensor, order: torch.Tensor, ptr: torch.Tensor, t_beta: float, t_d: float,
              lds_nodes: int = 0):
    """(local[N] int64, assoc[N] int64, nclusters[B] int64, flags[2] int32) of dmet_condense_f32 for beta[N], x[N, D] fp32
    and the ranking order[N] int64 (`_topk` over the score with non-candidates at -inf, out_ptr = ptr, M = N).  local: the
    event-local number of a node's condensation point, assoc: its global id, -1 both for noise.  flags: ranking entries
    outside their event | the walk reached its bound.  lds_nodes: the largest event kept in LDS (0: the default)."""
    dev = _require_device(beta, x, order, ptr)
    L = _lib.load()
    beta = _f32c(beta.detach(), "beta")
    x = _f32c(x.detach(), "x")
    if beta.dim() != 1 or x.dim() != 2 or x.shape[0] != beta.numel():
        raise ValueError(f"condense: beta must be [N] and x [N, D], got {tuple(beta.shape)} and {tuple(x.shape)}")
    N, D = x.shape
    order = _sel_vec(order, "order", torch.int64, N)
    ptr = _sel_vec(ptr, "ptr", torch.int64)
    if ptr.numel() < 1:
        raise TypeError("condense: ptr must hold B + 1 entries")
    B = ptr.numel() - 1
    local = torch.empty((N,), dtype=torch.int64, device=dev)
    assoc = torch.empty((N,), dtype=torch.int64, device=dev)
    nclusters = torch.empty((B,), dtype=torch.int64, device=dev)
    flags = torch.empty((2,), dtype=torch.int32, device=dev)
    _t = timer.record('condense', dev)
    with _on(dev):
        ws = _ws(L.dmet_condense_workspace_bytes(N), dev)
        _lib.check(L.dmet_condense_f32(_ptr(beta), _ptr(x), _ptr(order), ptr.data_ptr(), B, N, int(D), float(t_beta),
                                       float(t_d), _ptr(local), _ptr(assoc), _ptr(nclusters), flags.data_ptr(),
                                       int(lds_nodes), ws.data_ptr(), ws.numel(), _stream(dev)), "dmet_condense_f32")
    if _t is not None:
        _t.record(torch.cuda.current_stream(dev))
    return local, assoc, nclusters, flags

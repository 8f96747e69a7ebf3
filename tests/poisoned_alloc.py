"""Fill every tensor deepmetv2_amd._native allocates with torch.empty before the kernels see it.

`poisoned(pattern)` replaces the module global `torch` of deepmetv2_amd._native with a proxy that forwards every attribute to
the real torch and follows `empty` with a fill, for the duration of the block; the global is restored on exit, also on an
exception.  The fill does not depend on which block the caching allocator hands out: a kernel that leaves part of an output
unwritten, or reads a workspace word nothing wrote in the same call, returns different bits under the two patterns.

Patterns (both index-safe):

  ones        every byte 0xFF: fp32 / bf16 / fp16 read NaN, int16 / int32 / int64 read -1 (the project's own "no
              neighbour"), uint8 reads 255.
  zeros_huge  tensors allocated with a floating dtype hold +3.0e38 (65504 in fp16; finite: a max-aggregation that would
              silently drop a NaN cannot drop this); every other tensor, the raw uint8 workspaces included, holds byte 0x00.

There is deliberately NO pattern that makes an integer word an out-of-range index or a huge count.  A poisoned word is a
value every consumer already tolerates as an index (-1 or 0): an uninitialised index that left its allocation would fault
the card for everybody on it.  The point is to turn reads of uninitialised memory into wrong bits, not into faults -- add
no pattern that breaks this.

The proxy counts the allocations it filled (`Poison.count`); a case in which the count stays 0 poisoned nothing and is a
broken case."""
import contextlib

import torch

PATTERNS = ("ones", "zeros_huge")
HUGE = 3.0e38


def fill_(t: torch.Tensor, pattern: str) -> torch.Tensor:
    if t.numel() == 0:
        return t
    if pattern == "ones":
        t.view(-1).view(torch.uint8).fill_(0xFF)
    elif t.dtype.is_floating_point:
        t.fill_(min(HUGE, torch.finfo(t.dtype).max))       # fp16 cannot hold 3e38: its largest finite value
    else:
        t.view(-1).view(torch.uint8).zero_()
    return t


class Poison:
    """Stands in for the `torch` global of deepmetv2_amd._native: every attribute is the real torch's, `empty` fills."""

    def __init__(self, pattern: str):
        if pattern not in PATTERNS:
            raise ValueError(f"unknown poison pattern {pattern!r} (index-safe patterns only: {PATTERNS})")
        self.pattern = pattern
        self.count = 0        # allocations filled
        self.elements = 0     # ... and their elements

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        self.count += 1
        self.elements += t.numel()
        return fill_(t, self.pattern)

    def empty_like(self, ref, *args, **kwargs):
        t = torch.empty_like(ref, *args, **kwargs)
        self.count += 1
        self.elements += t.numel()
        return fill_(t, self.pattern)


@contextlib.contextmanager
def poisoned(pattern: str, module=None):
    """with poisoned("ones") as p: ...; p.count allocations of deepmetv2_amd._native were filled inside the block."""
    if module is None:
        from deepmetv2_amd import _native as module
    proxy = Poison(pattern)
    real = module.torch
    module.torch = proxy
    try:
        yield proxy
    finally:
        module.torch = real


def flatten(result):
    """The tensors of a wrapper's result, in order, through tuples / lists; None and non-tensors are skipped."""
    if isinstance(result, torch.Tensor):
        return [result]
    if isinstance(result, (tuple, list)):
        return [t for r in result for t in flatten(r)]
    return []


def to_bytes(t: torch.Tensor) -> torch.Tensor:
    """A CPU copy of t as uint8 [numel, itemsize]: what bitwise equality is taken over (NaN == NaN here)."""
    c = t.detach().cpu().contiguous()
    return c.view(-1).view(torch.uint8).view(c.numel(), c.element_size()) if c.numel() else torch.zeros((0, 1), dtype=torch.uint8)


def differing(a: torch.Tensor, b: torch.Tensor, keep=None) -> torch.Tensor:
    """Flat indices of the elements whose bytes differ between a and b, among those `keep` (bool, a's shape) retains."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    diff = (to_bytes(a) != to_bytes(b)).any(dim=1)
    if keep is not None:
        diff &= keep.reshape(-1).cpu()
    return diff.nonzero().view(-1)


def run_both(call):
    """call() under each pattern: {pattern: list of CPU tensors}; fails if a run poisoned nothing."""
    out = {}
    for pattern in PATTERNS:
        with poisoned(pattern) as p:
            res = call()
        assert p.count > 0, f"no allocation was poisoned under {pattern!r}: the case does not reach _native's torch.empty"
        out[pattern] = [t.detach().cpu() for t in flatten(res)]
    return out

"""The seven radius entries of the C ABI (include/dmet.h), each called directly through _lib.load().

nbr / cnt, and nbr16 where the entry has one, for equality with the numpy restatements (tests/radius_periodic_reference.py
for one point set, tests/knn_xy_reference.py for two) at both edges of every rung of the D ladder, on events that put a
wavefront across events, an empty and a one-node event and events one over the 64-lane and 128-entry boundaries of the
window kernel, with a cap that ends rows inside the first 4-id slot (max_nbr = 3) and inside the second 8-id slot of the
uint16 rows (max_nbr = 9, stride16 = 16)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import knn_xy_reference as xy
import radius_periodic_reference as rp
from test_gpu_radius_periodic import _expected_rows16

pytestmark = pytest.mark.gpu

SIZES = [63, 0, 1, 65, 130]        # candidates, and the queries of the one-set entries
QSIZES = [5, 3, 0, 70, 64]         # queries of the two-set entry
R = 0.4
DS = [1, 2, 3, 4, 5, 8]
CAPS = [3, 9]
POISON = 2 ** 30                   # every slot of a table before the call
POISON16 = 0x1234


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _side(D):
    """Box side at which a ball of radius R holds about 20 of the 130 nodes of the last event (fewer near the faces):
    the cap of 3 and of 9 binds there; also the circumference of a periodic coordinate."""
    ball = math.pi ** (D / 2) / math.gamma(D / 2 + 1) * R ** D
    return float(np.float32((130 * ball / 20) ** (1 / D)))


@functools.lru_cache(maxsize=None)
def _points(D, n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((n, D), dtype=np.float32) - np.float32(0.5)) * np.float32(_side(D))).astype(np.float32)


def _period(D, kind):
    """D floats: all 0 ("none"), or the box side on the last ("last") or the first ("first") coordinate."""
    per = [0.0] * D
    if kind != "none":
        per[D - 1 if kind == "last" else 0] = _side(D)
    return per


@functools.lru_cache(maxsize=None)
def _hits(D, kind):
    return rp.radius_hits(_points(D, sum(SIZES), 100 + D), _ptr(SIZES), R, _period(D, kind))


def _want(D, kind, m, skip):
    """The reference table; the cap binds in the 130-node event and leaves other rows short."""
    nbr, cnt = rp.cap(_hits(D, kind), m, skip_self=bool(skip))
    assert (cnt[-130:] == m).any() and (cnt < m).any(), (D, kind, m, skip, int(cnt.max()))
    return nbr, cnt


class _Run:
    """Device operands of one (D, max_nbr) and the direct calls on them."""

    def __init__(self, dev, D, m):
        from deepmetv2_amd import _lib, _native
        self.dev, self.D, self.m, self.L = dev, D, m, _lib.load()
        self.check = _lib.check
        self.st = _native._stream(dev)
        self.N, self.B = sum(SIZES), len(SIZES)
        self.x = torch.from_numpy(_points(D, self.N, 100 + D)).to(dev)
        self.ptr = torch.from_numpy(_ptr(SIZES)).to(dev)
        self.stride16 = (m + 7) // 8 * 8
        self.ws = torch.empty((self.L.dmet_radius_workspace_bytes(self.N),), dtype=torch.uint8, device=dev)

    def tables(self, n, want_nbr=True, want_nbr16=False):
        nbr = torch.full((n, self.m), POISON, dtype=torch.int32, device=self.dev) if want_nbr else None
        cnt = torch.full((n,), POISON, dtype=torch.int32, device=self.dev)
        nbr16 = torch.full((n, self.stride16), POISON16, dtype=torch.int16, device=self.dev) if want_nbr16 else None
        return nbr, cnt, nbr16

    def one_set(self, entry, skip, fill, kind="none", want_nbr=True, want_nbr16=False):
        """Call a one-set entry; (nbr, cnt, nbr16) as CPU tensors, None where the call had none."""
        nbr, cnt, nbr16 = self.tables(self.N, want_nbr, want_nbr16)
        per = (ctypes.c_float * self.D)(*_period(self.D, kind))
        per_p = ctypes.cast(per, ctypes.c_void_p)
        p = lambda t: None if t is None else t.data_ptr()
        head = (self.x.data_ptr(), self.ptr.data_ptr(), self.B, self.N, self.D, R, self.m, skip)
        out = (p(nbr), cnt.data_ptr())
        rows = (p(nbr16), self.stride16 if want_nbr16 else 0)
        ws = (self.ws.data_ptr(), self.ws.numel(), self.st)
        args = {
            "dmet_radius_f32": (*head, *out, self.st),
            "dmet_radius_counted_f32": (*head, *out, self.st),
            "dmet_radius_windowed_f32": (*head, fill, *out, *ws),
            "dmet_radius_windowed_local_f32": (*head, fill, *out, *rows, *ws),
            "dmet_radius_periodic_f32": (*head, fill, per_p, *out, self.st),
            "dmet_radius_windowed_periodic_f32": (*head, fill, per_p, *out, *rows, *ws),
        }[entry]
        self.check(getattr(self.L, entry)(*args), entry)
        return tuple(None if t is None else t.cpu() for t in (nbr, cnt, nbr16))


def _compare(got, want_nbr, want_cnt, fill, ptr, what):
    """cnt; nbr whole (fill) or in its slots < cnt; nbr16 in its slots < roundup8(cnt) (ids, then 0xFFFF)."""
    nbr, cnt, nbr16 = got
    want_nbr, want_cnt = torch.from_numpy(want_nbr), torch.from_numpy(want_cnt)
    assert torch.equal(cnt, want_cnt), what
    if nbr is not None:
        keep = torch.arange(want_nbr.shape[1]).view(1, -1) < want_cnt.view(-1, 1)
        assert torch.equal(nbr[keep], want_nbr[keep]), what
        if fill:
            assert torch.equal(nbr, want_nbr), what
    if nbr16 is not None:
        loc, written = _expected_rows16(want_nbr, want_cnt, torch.from_numpy(ptr), nbr16.shape[1])
        assert torch.equal(nbr16[written], loc[written]), what


@pytest.mark.parametrize("m", CAPS)
@pytest.mark.parametrize("D", DS)
def test_plain_entries(dev, D, m):
    run, ptr = _Run(dev, D, m), _ptr(SIZES)
    for skip in (0, 1):
        want = _want(D, "none", m, skip)
        _compare(run.one_set("dmet_radius_f32", skip, 1), *want, 1, ptr, ("f32", skip))
        _compare(run.one_set("dmet_radius_counted_f32", skip, 0), *want, 0, ptr, ("counted", skip))
        for fill in (0, 1):
            _compare(run.one_set("dmet_radius_windowed_f32", skip, fill), *want, fill, ptr, ("windowed", skip, fill))
            _compare(run.one_set("dmet_radius_windowed_local_f32", skip, fill, want_nbr16=True), *want, fill, ptr,
                     ("windowed_local", skip, fill))
        _compare(run.one_set("dmet_radius_windowed_local_f32", skip, 0, want_nbr=False, want_nbr16=True), *want, 0, ptr,
                 ("windowed_local, nbr = NULL", skip))


@pytest.mark.parametrize("m", CAPS)
@pytest.mark.parametrize("D", DS)
def test_periodic_entries(dev, D, m):
    run, ptr = _Run(dev, D, m), _ptr(SIZES)
    win_kind = "last" if D > 1 else "none"        # the window runs on coordinate 0: D = 1 has no other to wrap
    for skip in (0, 1):
        for fill in (0, 1):
            for kind in sorted({"last" if D > 1 else "first", "first"}):
                _compare(run.one_set("dmet_radius_periodic_f32", skip, fill, kind), *_want(D, kind, m, skip), fill, ptr,
                         ("periodic", kind, skip, fill))
            want = _want(D, win_kind, m, skip)
            for rows in (False, True):
                _compare(run.one_set("dmet_radius_windowed_periodic_f32", skip, fill, win_kind, want_nbr16=rows), *want,
                         fill, ptr, ("windowed_periodic", rows, skip, fill))
        _compare(run.one_set("dmet_radius_windowed_periodic_f32", skip, 0, win_kind, want_nbr=False, want_nbr16=True),
                 *_want(D, win_kind, m, skip), 0, ptr, ("windowed_periodic, nbr = NULL", skip))


@pytest.mark.parametrize("m", CAPS)
@pytest.mark.parametrize("D", DS)
def test_two_set_entry(dev, D, m):
    run = _Run(dev, D, m)
    Ny, ptr_y = sum(QSIZES), _ptr(QSIZES)
    y = _points(D, Ny, 200 + D)
    yd, pyd = torch.from_numpy(y).to(dev), torch.from_numpy(ptr_y).to(dev)
    for kind in (None, "last"):
        period = None if kind is None else _period(D, kind)
        want_nbr, want_cnt = xy.radius_table(_points(D, run.N, 100 + D), _ptr(SIZES), y, ptr_y, R, m, period)
        assert (want_cnt == m).any() and (want_cnt < m).any(), (D, kind, m)
        per = None if period is None else (ctypes.c_float * D)(*period)
        for fill in (0, 1):
            nbr, cnt, _ = run.tables(Ny)
            run.check(run.L.dmet_radius_xy_f32(run.x.data_ptr(), run.ptr.data_ptr(), run.N, yd.data_ptr(), pyd.data_ptr(),
                                               Ny, run.B, D, R, m, None if per is None else ctypes.cast(per, ctypes.c_void_p),
                                               fill, nbr.data_ptr(), cnt.data_ptr(), run.st), "dmet_radius_xy_f32")
            _compare((nbr.cpu(), cnt.cpu(), None), want_nbr, want_cnt, fill, ptr_y, ("xy", kind, fill))

"""radius_graph(..., period=): host-side checks of the periodic radius graph (no GPU needed).

The argument validation, the routing of a plain `period` to the unchanged build, the choice between the windowed and
the all-pairs entry, the C entries' own argument checks, and the numpy restatement against exact rationals."""
import contextlib
import ctypes
import math
import os
import shutil

import numpy as np
import pytest
import torch

import radius_periodic_reference as rp

TWO_PI_F32 = float(np.float32(2 * math.pi))


def _events(seed=0, sizes=(40, 0, 7, 25)):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    x = torch.stack([(torch.rand(N, generator=g) - 0.5) * 4, (torch.rand(N, generator=g) - 0.5) * 6.28], 1)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return x, batch


# ---- validation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period,exc", [
    ([2 * math.pi], ValueError),                        # length != D
    ([None, 2 * math.pi, None], ValueError),
    ([None, float("nan")], ValueError),
    ([None, float("inf")], ValueError),
    ([None, -1.0], ValueError),
    ([None, 1e-60], ValueError),                        # rounds to 0 in fp32
    ([None, 1e39], ValueError),                         # rounds to inf in fp32
    ([None, True], TypeError),
    ([None, "6.28"], TypeError),
    ([None, torch.tensor(6.28)], TypeError),
    ("ab", TypeError),
    (6.28, TypeError),
    ({0: None, 1: 6.28}, TypeError),
])
def test_bad_period_is_rejected_before_any_device_work(monkeypatch, period, exc):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native

    def boom(*a, **k):
        raise AssertionError("a native entry ran although the period is invalid")

    monkeypatch.setattr(_native, "radius", boom)
    monkeypatch.setattr(_native, "radius_periodic", boom)
    x, batch = _events()
    with pytest.raises(exc):
        dm.radius_table(x, 0.4, batch, loop=True, max_num_neighbors=16, period=period)
    with pytest.raises(exc):
        dm.radius_graph(x, 0.4, batch, loop=True, max_num_neighbors=16, period=period)


def test_period_is_rounded_to_fp32():
    from deepmetv2_amd.cluster import _check_period
    assert _check_period([None, 2 * math.pi], 2) == [0.0, TWO_PI_F32]
    assert _check_period((0, np.float64(6.0)), 2) == [0.0, 6.0]
    assert _check_period([None, None], 2) is None
    assert _check_period([0, 0.0], 2) is None
    assert _check_period(None, 2) is None


# ---- routing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [None, [None, None], [0, 0], [0.0, None]])
def test_plain_period_calls_the_unchanged_radius(monkeypatch, period):
    """None / all-zero: _native.radius with exactly the arguments of a call without `period`, same table."""
    import fake_native
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    fake_native.install(monkeypatch)
    calls = []

    def spy(*a, **k):
        calls.append((a, k))
        return fake_native.radius(*a, **k)

    def boom(*a, **k):
        raise AssertionError("the periodic entry ran for a plain period")

    monkeypatch.setattr(_native, "radius", spy)
    monkeypatch.setattr(_native, "radius_periodic", boom)
    x, batch = _events(1)
    for loop in (True, False):
        calls.clear()
        t0 = dm.radius_table(x, 0.4, batch, loop=loop, max_num_neighbors=16)
        t1 = dm.radius_table(x, 0.4, batch, loop=loop, max_num_neighbors=16, period=period)
        assert len(calls) == 2
        (a0, k0), (a1, k1) = calls
        assert len(a0) == len(a1) and all((u is v) or (torch.is_tensor(u) and torch.equal(u, v)) or u == v
                                          for u, v in zip(a0, a1))
        assert k0 == k1
        assert torch.equal(t0.edge_index(), t1.edge_index())
        e0 = dm.radius_graph(x, 0.4, batch, loop=loop, max_num_neighbors=16)
        e1 = dm.radius_graph(x, 0.4, batch, loop=loop, max_num_neighbors=16, period=period)
        assert torch.equal(e0, e1)


def test_periodic_call_reaches_radius_periodic(monkeypatch):
    import fake_native
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    fake_native.install(monkeypatch)
    seen = {}

    def spy(x, ptr, r, m, skip_self=False, pad=True, local=False, int32_rows=True, period=None):
        seen.update(period=period, skip_self=skip_self, pad=pad, local=local, m=m)
        nbr, cnt = rp.radius_table(x.numpy(), ptr.numpy(), r, m, period, skip_self)
        return torch.from_numpy(nbr), torch.from_numpy(cnt), None

    monkeypatch.setattr(_native, "radius", spy)     # radius_table hands the periods to the one entry, as period=
    x, batch = _events(2)
    ei = dm.radius_graph(x, 0.4, batch, loop=False, max_num_neighbors=8, period=[None, 2 * math.pi])
    assert seen == dict(period=[0.0, TWO_PI_F32], skip_self=True, pad=False, local=True, m=9)
    assert ei.shape[0] == 2 and ei.dtype == torch.int64


class _FakeLib:
    """Records which C entry _native.radius_periodic calls (and the periods it hands over)."""

    def __init__(self):
        self.calls = []

    def dmet_radius_workspace_bytes(self, N):
        return 4 * N + 512

    def dmet_radius_periodic_f32(self, *a):
        per = ctypes.cast(a[9], ctypes.POINTER(ctypes.c_float))
        self.calls.append(("all_pairs", [per[c] for c in range(a[4])], a))
        return 0

    def dmet_radius_windowed_periodic_f32(self, *a):
        per = ctypes.cast(a[9], ctypes.POINTER(ctypes.c_float))
        self.calls.append(("windowed", [per[c] for c in range(a[4])], a))
        return 0


@pytest.mark.parametrize("form", ["windowed", "sweep"])
@pytest.mark.parametrize("period", [[0.0, TWO_PI_F32], [TWO_PI_F32, 0.0], [TWO_PI_F32, TWO_PI_F32]])
def test_coordinate0_periodic_selects_all_pairs(monkeypatch, form, period):
    from deepmetv2_amd import _lib, _native
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_native, "_require_device", lambda *t: torch.device("cpu"))
    monkeypatch.setattr(_native, "_stream", lambda dev: None)
    monkeypatch.setattr(_native, "_on", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(_native, "RADIUS_FORM", form)
    x, _ = _events(3)
    ptr = torch.tensor([0, x.shape[0]], dtype=torch.int64)
    nbr, cnt, rows16 = _native.radius_periodic(x, ptr, 0.4, 32, period, pad=False, local=True, int32_rows=False)
    want = "windowed" if (form == "windowed" and period[0] == 0.0) else "all_pairs"
    assert [c[0] for c in fake.calls] == [want]
    assert fake.calls[0][1] == [np.float32(p) for p in period]
    assert (rows16 is None) == (want == "all_pairs")
    assert (nbr is None) == (want == "windowed")     # int32_rows=False skips the int32 table where the form can
    fake.calls.clear()
    out = _native.radius_periodic(x, ptr, 0.4, 32, period, skip_self=True, pad=True)
    assert len(out) == 2 and [c[0] for c in fake.calls] == [want]


# ---- the C entries' own checks (no GPU touched: every one fails before a HIP call) -------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def _per(*v):
    arr = (ctypes.c_float * len(v))(*v)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_abi_rejects_bad_periods(lib):
    nan, inf = float("nan"), float("inf")
    for vals in [(0.0, nan), (0.0, inf), (0.0, -1.0), (-inf, 0.0)]:
        keep, p = _per(*vals)
        assert lib.dmet_radius_periodic_f32(None, None, 1, 10, 2, 0.4, 32, 0, 0, p, None, None, None) == -22
        assert b"period" in lib.dmet_last_error()
        assert lib.dmet_radius_windowed_periodic_f32(None, None, 1, 10, 2, 0.4, 32, 0, 0, p, None, None, None, 0,
                                                     None, 0, None) == -22
    keep, p = _per(0.0, 6.28)
    for D in (0, 9):
        assert lib.dmet_radius_periodic_f32(None, None, 1, 10, D, 0.4, 32, 0, 0, p, None, None, None) == -22
        assert b"D=" in lib.dmet_last_error()
        assert lib.dmet_radius_windowed_periodic_f32(None, None, 1, 10, D, 0.4, 32, 0, 0, p, None, None, None, 0,
                                                     None, 0, None) == -22
    assert lib.dmet_radius_periodic_f32(None, None, 1, 10, 2, 0.4, 32, 0, 0, None, None, None, None) == -22
    assert b"null period" in lib.dmet_last_error()
    assert lib.dmet_radius_windowed_periodic_f32(None, None, 1, 10, 2, 0.4, 32, 0, 0, None, None, None, None, 0,
                                                 None, 0, None) == -22
    # the window runs on coordinate 0: a periodic coordinate 0 is refused there (also for D = 1)
    keep, p = _per(6.28, 0.0)
    assert lib.dmet_radius_windowed_periodic_f32(None, None, 1, 10, 2, 0.4, 32, 0, 0, p, None, None, None, 0,
                                                 None, 0, None) == -22
    assert b"coordinate 0" in lib.dmet_last_error()
    keep, p = _per(6.28)
    assert lib.dmet_radius_windowed_periodic_f32(None, None, 1, 10, 1, 0.4, 32, 0, 0, p, None, None, None, 0,
                                                 None, 0, None) == -22
    # valid periods, null buffers: the plain entries' own checks apply; an empty problem is a no-op
    keep, p = _per(0.0, 6.28)
    assert lib.dmet_radius_periodic_f32(None, None, 1, 10, 2, 0.4, 32, 0, 0, p, None, None, None) == -22
    assert lib.dmet_radius_periodic_f32(None, None, 1, 10, 2, 0.4, 0, 0, 0, p, None, None, None) == -22
    assert lib.dmet_radius_periodic_f32(None, None, 0, 0, 2, 0.4, 32, 0, 0, p, None, None, None) == 0
    assert lib.dmet_radius_windowed_periodic_f32(None, None, 0, 0, 2, 0.4, 32, 0, 0, p, None, None, None, 0,
                                                 None, 0, None) == 0


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_reference_fma_is_exact_against_fractions():
    g = np.random.default_rng(5)
    L = TWO_PI_F32
    xs = [(g.random((400, 3)) - 0.5) * np.array([10.0, 2 * L, 1e-3]),
          np.round((g.random((200, 3)) - 0.5) * 8) / 4 * np.array([1, L / 8 * 4, 1])]
    edge = np.float32(np.pi)
    xs.append(np.array([[0, edge, 0], [0, -edge, 0], [1e-3, 0.0, 5], [0.4, L / 2, -5], [3e3, -L / 2, 1e-7]]))
    for x in xs:
        x = x.astype(np.float32)
        for period in ([None, L, None], [L, L, None], None, [None, 1.0, 0.5]):
            i = g.integers(0, len(x), 300)
            j = g.integers(0, len(x), 300)
            got = rp.pair_d2(x[i], x[j], period)
            want = np.array([rp.fraction_pair_d2(x[a], x[b], period) for a, b in zip(i, j)], dtype=np.float32)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), period


def test_reference_fma_rounds_where_float64_would_not():
    # a*a + acc with a 48-bit product whose low bits decide the fp32 rounding: the restatement must round once
    a = np.float32(1 + 2 ** -12)
    acc = np.float32(2 ** -23 + 2 ** -46)     # representable: 24 bits from 2^-23
    got = rp._fma32(np.array([a]), np.array([acc]))[0]
    want = rp.round_f32(rp.Fraction(float(a)) ** 2 + rp.Fraction(float(acc)))
    assert got == np.float32(want)


def test_reference_wraps_at_the_seam():
    L = TWO_PI_F32
    x = np.array([[0.0, np.float32(np.pi)], [0.0, -np.float32(np.pi)], [0.0, 3.1], [0.0, -3.1], [0.0, 0.0]], np.float32)
    ptr = np.array([0, 5])
    nbr, cnt = rp.radius_table(x, ptr, 0.4, 8, [None, L])
    assert [sorted(nbr[i, :cnt[i]].tolist()) for i in range(5)] == [[0, 1, 2, 3]] * 4 + [[4]]
    nbr0, cnt0 = rp.radius_table(x, ptr, 0.4, 8, None)
    assert cnt0.tolist() == [2, 2, 2, 2, 1]

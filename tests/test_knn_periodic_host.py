"""knn_table / knn_graph / knn(..., period=): host-side checks of the periodic kNN graph (no GPU needed).

The argument validation before any device work, the routing of a plain `period` to the unchanged build, the periodic
call's arguments, the C entry's own checks, and the numpy restatement against the oracle and exact rationals."""
import ctypes
import math
import os
import shutil

import numpy as np
import pytest
import torch

import knn_periodic_reference as kp
import radius_periodic_reference as rp

TWO_PI_F32 = float(np.float32(2 * math.pi))


def _events(seed=0, sizes=(40, 0, 7, 25)):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    x = torch.stack([(torch.rand(N, generator=g) - 0.5) * 4, (torch.rand(N, generator=g) - 0.5) * 6.28], 1)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return x, batch


def _no_native(monkeypatch):
    from deepmetv2_amd import _native

    def boom(*a, **k):
        raise AssertionError("a native entry ran although the arguments are invalid")

    for n in ("knn", "knn_local", "knn_local_dense", "knn_periodic", "knn_size_hint"):
        monkeypatch.setattr(_native, n, boom)


# ---- validation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period,exc,msg", [
    ([2 * math.pi], ValueError, "entries"),                        # length != D
    ([None, 2 * math.pi, None], ValueError, "entries"),
    ([None, float("nan")], ValueError, "positive finite"),
    ([None, float("inf")], ValueError, "positive finite"),
    ([None, -1.0], ValueError, "positive finite"),
    ([None, 1e-60], ValueError, "positive finite"),                # rounds to 0 in fp32
    ([None, 1e39], ValueError, "positive finite"),                 # rounds to inf in fp32
    ([None, True], TypeError, "period\\[1\\]"),
    ([None, "6.28"], TypeError, "period\\[1\\]"),
    ([None, torch.tensor(6.28)], TypeError, "period\\[1\\]"),
    ("ab", TypeError, "period must be"),
    (6.28, TypeError, "period must be"),
])
def test_bad_period_is_rejected_before_any_device_work(monkeypatch, period, exc, msg):
    import deepmetv2_amd as dm
    _no_native(monkeypatch)
    x, batch = _events()
    for loop in (True, False):
        with pytest.raises(exc, match=msg):
            dm.knn_table(x, 8, batch, loop=loop, period=period)
        with pytest.raises(exc, match=msg):
            dm.knn_graph(x, 8, batch, loop=loop, period=period)
    with pytest.raises(exc, match=msg):
        dm.knn(x, x, 8, batch, batch, period=period)


def test_more_than_8_coordinates_with_a_period_is_rejected(monkeypatch):
    import deepmetv2_amd as dm
    _no_native(monkeypatch)
    x = torch.zeros(10, 9)
    period = [None] * 8 + [6.28]
    with pytest.raises(ValueError, match="up to 8 coordinates"):
        dm.knn_table(x, 4, period=period)
    with pytest.raises(ValueError, match="up to 8 coordinates"):
        dm.knn_graph(x, 4, loop=True, period=period)


# ---- routing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [None, [None, None], [0, 0], [0.0, None]])
def test_plain_period_calls_the_unchanged_knn(monkeypatch, period):
    """None / all-zero: the plain native entries with exactly the arguments of a call without `period`, same table."""
    import fake_native
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    fake_native.install(monkeypatch)
    calls = []

    def spy(name):
        f = getattr(fake_native, name)

        def g(*a, **k):
            calls.append((name, a, k))
            return f(*a, **k)
        return g

    def boom(*a, **k):
        raise AssertionError("the periodic entry ran for a plain period")

    monkeypatch.setattr(_native, "knn", spy("knn"))
    monkeypatch.setattr(_native, "knn_local", spy("knn_local"))
    monkeypatch.setattr(_native, "knn_periodic", boom)
    x, batch = _events(1)
    for loop, k in ((True, 8), (True, 5), (False, 8)):
        calls.clear()
        t0 = dm.knn_table(x, k, batch, loop=loop)
        t1 = dm.knn_table(x, k, batch, loop=loop, period=period)
        assert len(calls) == 2
        (n0, a0, k0), (n1, a1, k1) = calls
        assert n0 == n1 and k0 == k1 and len(a0) == len(a1)
        assert all((u is v) or (torch.is_tensor(u) and torch.equal(u, v)) or u == v for u, v in zip(a0, a1))
        assert torch.equal(t0.nbr, t1.nbr) and torch.equal(t0.dist, t1.dist)
        e0 = dm.knn_graph(x, k, batch, loop=loop)
        e1 = dm.knn_graph(x, k, batch, loop=loop, period=period)
        assert torch.equal(e0, e1)
    assert torch.equal(dm.knn(x, x, 8, batch, batch), dm.knn(x, x, 8, batch, batch, period=period))


@pytest.mark.parametrize("loop,k,local", [(True, 16, True), (True, 5, False), (False, 16, False), (False, 7, False)])
def test_periodic_call_reaches_knn_periodic(monkeypatch, loop, k, local):
    """The periodic entry gets the fp32 periods and the searched width; the event-local ids are asked for exactly where
    a plain build asks for them (loop=True, k in LDS_GATHER_K), and loop=False blanks the node itself."""
    import fake_native
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    fake_native.install(monkeypatch)
    seen = {}

    def spy(x, ptr, kk, period, want_local):
        seen.update(period=period, k=kk, want_local=want_local)
        nbr, dist, loc = kp.knn_table(x.numpy(), ptr.numpy(), kk, period)
        return (torch.from_numpy(nbr), torch.from_numpy(dist),
                torch.from_numpy(loc.view(np.int16)) if want_local else None)

    monkeypatch.setattr(_native, "knn_periodic", spy)
    x, batch = _events(2)
    table = dm.knn_table(x, k, batch, loop=loop, period=[None, 2 * math.pi])
    kk = k if loop else k + 1
    assert seen == dict(period=[0.0, TWO_PI_F32], k=kk, want_local=local)
    assert (table.nbr_local is not None) == local
    ptr = torch.tensor([0, 40, 40, 47, 72])
    want, _, _ = kp.knn_table(x.numpy(), ptr.numpy(), kk, [None, TWO_PI_F32])
    if not loop:
        want = np.where(want == np.arange(x.shape[0])[:, None], -1, want)
    assert np.array_equal(table.nbr.numpy(), want)
    ei = dm.knn_graph(x, k, batch, loop=loop, period=[None, 2 * math.pi])
    assert ei.shape[0] == 2 and ei.dtype == torch.int64
    assert int((ei[0] >= 0).sum()) == ei.shape[1]


def test_dynamic_edgeconv_has_no_period():
    import inspect
    from deepmetv2_amd import conv
    if hasattr(conv, "DynamicEdgeConv"):
        assert "period" not in inspect.signature(conv.DynamicEdgeConv.__init__).parameters


# ---- the C entry's own checks (no GPU touched: every one fails before a HIP call) --------------------------------
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
    args = lambda D, p: (None, None, 1, 10, D, 8, p, None, None, None, None, 0, None)   # noqa: E731
    for vals in [(0.0, nan), (0.0, inf), (0.0, -1.0), (-inf, 0.0), (-0.5,)]:
        keep, p = _per(*vals)
        assert lib.dmet_knn_periodic_f32(*args(len(vals), p)) == -22
        assert b"period" in lib.dmet_last_error()
    keep, p = _per(*([0.0] * 8 + [6.28]))
    for D in (0, 9, 32):
        assert lib.dmet_knn_periodic_f32(*args(D, p)) == -22
        assert b"D=" in lib.dmet_last_error()
    assert lib.dmet_knn_periodic_f32(*args(2, None)) == -22
    assert b"null period" in lib.dmet_last_error()
    # valid periods, null buffers: the plain entry's own checks apply; an empty problem is a no-op
    keep, p = _per(0.0, 6.28)
    assert lib.dmet_knn_periodic_f32(*args(2, p)) == -22
    assert b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_knn_periodic_f32(None, None, 1, 10, 2, 0, p, None, None, None, None, 0, None) == -22
    assert lib.dmet_knn_periodic_f32(None, None, 0, 0, 2, 8, p, None, None, None, None, 0, None) == 0
    keep, p = _per(0.0, 0.0)       # all zero: the plain entry, same checks
    assert lib.dmet_knn_periodic_f32(*args(2, p)) == -22
    assert b"null pointer" in lib.dmet_last_error()


def test_abi_output_flags_are_stored_before_the_first_check(lib):
    """dense_done / fused are written as 0 before any argument check, so a caller never reads a stale 1 after a
    refused or an ineligible call (all of these return before a HIP call)."""
    def flag():
        v = ctypes.c_int(7)
        return v, ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)
    # dmet_knn_local_dense_f32(x, ptr, B, N, D, k, nbr, dist, nbr16, W, bias, layout, P, Q, dense_done, ws, ws_bytes, stream)
    done, done_p = flag()
    assert lib.dmet_knn_local_dense_f32(None, None, 1, 10, 32, 8, None, None, None, None, None, 0, None, None, done_p,
                                        None, 0, None) == -22
    assert b"null pointer" in lib.dmet_last_error() and done.value == 0
    # dmet_bn_knn_local_dense_f32(raw, residual, gamma, beta, mean, invstd, y, ptr, B, N, D, k, nbr, dist, nbr16, W, bias,
    #                             layout, P, Q, dense_done, fused, ws, ws_bytes, stream)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    done, done_p = flag()
    fused, fused_p = flag()
    assert lib.dmet_bn_knn_local_dense_f32(p, None, p, p, p, p, p, None, 1, 10, 16, 8, None, None, None, None, None, 0,
                                           None, None, done_p, fused_p, None, 0, None) == 0        # D != 32: not eligible
    assert fused.value == 0 and done.value == 0
    done, done_p = flag()
    fused, fused_p = flag()
    assert lib.dmet_bn_knn_local_dense_f32(p, None, None, p, p, p, p, None, 1, 10, 32, 8, None, None, None, None, None, 0,
                                           None, None, done_p, fused_p, None, 0, None) == -22      # null gamma
    assert b"null pointer" in lib.dmet_last_error() and fused.value == 0 and done.value == 0


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_reference_matches_the_oracle_on_plain_inputs():
    from oracle import ref_ops
    g = np.random.default_rng(7)
    for D, k in ((1, 4), (2, 8), (3, 16), (8, 5)):
        x = ((g.random((90, D)) - 0.5) * 4).astype(np.float32)
        x[5] = x[6]                                     # exact ties
        x[10, 0] = np.nan
        x[11, 0] = np.inf
        ptr = np.array([0, 0, 1, 33, 90])
        nbr, dist, loc = kp.knn_table(x, ptr, k, None)
        nr, dr = ref_ops.knn_table(torch.from_numpy(x), torch.from_numpy(ptr), k)
        assert np.array_equal(nbr, nr.numpy())
        assert np.array_equal(dist.view(np.int32), dr.numpy().view(np.int32))
        lo = np.repeat(ptr[:-1], np.diff(ptr))[:, None]
        assert np.array_equal(loc, np.where(nbr >= 0, nbr - lo, 0xFFFF).astype(np.uint16))
        # an all-zero period is the plain table
        assert np.array_equal(kp.knn_table(x, ptr, k, [0.0] * D)[0], nbr)


def test_reference_distances_match_fractions():
    g = np.random.default_rng(9)
    L = TWO_PI_F32
    x = np.concatenate([(g.random((30, 2)) - 0.5) * np.array([5.0, 2 * L]),
                        [[0.0, np.float32(np.pi)], [0.0, -np.float32(np.pi)], [0.1, L / 2], [0.2, -L / 2]]])
    x = x.astype(np.float32)
    period = [None, L]
    nbr, dist, _ = kp.knn_table(x, np.array([0, len(x)]), 6, period)
    for i in range(0, len(x), 3):
        for s in range(6):
            j = nbr[i, s]
            assert dist[i, s] == np.float32(rp.fraction_pair_d2(x[i], x[j], period))


def test_reference_wraps_at_the_seam():
    L = TWO_PI_F32
    pi32 = np.float32(np.pi)
    x = np.array([[0.0, pi32], [0.0, -pi32], [0.0, 3.1], [0.0, -3.1], [0.0, 0.0], [0.0, 1.0]], np.float32)
    nbr, dist, _ = kp.knn_table(x, np.array([0, 6]), 3, [None, L])
    # +pi_f32 and -pi_f32 are at distance exactly 0: node 1 ties with node 0 and R2 puts the lower id first
    assert nbr[1].tolist()[:2] == [0, 1] and dist[1, 0] == 0 and dist[1, 1] == 0
    assert sorted(nbr[2].tolist()) == [0, 1, 2] and sorted(nbr[3].tolist()) == [0, 1, 3]
    plain, _, _ = kp.knn_table(x, np.array([0, 6]), 3, None)
    assert 3 not in plain[2].tolist()


def test_reference_geometry_is_the_circular_knn():
    g = np.random.default_rng(11)
    L = TWO_PI_F32
    x = np.stack([(g.random(300) - 0.5) * 5, (g.random(300) - 0.5) * L * 0.999], 1).astype(np.float32)
    nbr, _, _ = kp.knn_table(x, np.array([0, 300]), 8, [None, L])
    d64 = kp.circular_d2_f64(x, [None, L])
    for i in range(300):
        srt = np.sort(d64[i])
        if srt[8] - srt[7] < 1e-5:                    # too close to call in fp32
            continue
        assert set(nbr[i].tolist()) == set(np.argsort(d64[i], kind="stable")[:8].tolist())

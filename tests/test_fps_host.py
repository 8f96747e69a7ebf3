"""Farthest point sampling without a GPU: the numpy restatement of the contract (tests/fps_reference.py) against a float64
brute force and a hand-worked tie case, argument validation of the C entries (include/dmet.h "Farthest point sampling"),
and the Python-level errors of deepmetv2_amd.fps / nearest."""
import os
import shutil

import numpy as np
import pytest
import torch

import fps_reference as ref


def _greedy_f64(x, m, start):
    """The textbook greedy in float64; also the smallest relative gap between the best and the second-best candidate."""
    x = x.astype(np.float64)
    dist = ((x - x[start]) ** 2).sum(1)
    picks, gap = [start], np.inf
    for _ in range(1, m):
        order = np.argsort(-dist, kind="stable")
        gap = min(gap, (dist[order[0]] - dist[order[1]]) / dist[order[0]])
        s = int(order[0])
        picks.append(s)
        dist = np.minimum(dist, ((x - x[s]) ** 2).sum(1))
    return np.array(picks, dtype=np.int64), gap


@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_reference_matches_float64_greedy_without_ties(D):
    rng = np.random.default_rng(10 + D)
    sizes = [60, 1, 37]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = rng.standard_normal((int(ptr[-1]), D)).astype(np.float32)
    m = np.array([30, 1, 19])
    start = np.array([7, 0, 36])
    want = []
    for b, n in enumerate(sizes):
        picks, gap = _greedy_f64(x[ptr[b]:ptr[b + 1]], int(m[b]), int(start[b]))
        assert gap > 1e-5, "the input is meant to be tie-free far beyond fp32 rounding (2^-24 per fma)"
        want.append(picks + ptr[b])
    got = ref.fps(x, ptr, m, start)
    assert got.dtype == np.int64 and np.array_equal(got, np.concatenate(want))


def test_reference_tie_rule_on_a_lattice():
    """3 x 3 integer lattice, node 3 i + j at (i, j), start 0.  By hand: the far corner 8; then 2 and 6 tie at 4 -> 2, then
    6; the centre 4 (distance 2); then the four edge midpoints tie at 1 -> 1, 3, 5, 7 in index order; then every distance
    is 0 and index 0 repeats."""
    x = np.array([[i, j] for i in range(3) for j in range(3)], dtype=np.float32)
    got = ref.fps(x, [0, 9], [11], [0])
    assert got.tolist() == [0, 8, 2, 6, 4, 1, 3, 5, 7, 0, 0]
    # the start is clamped into the event; a second event is offset by its first node
    got = ref.fps(np.concatenate([x, x]), [0, 9, 18], [2, 3], [99, -5])
    assert got.tolist() == [8, 0, 9, 17, 11]


def test_reference_sample_counts():
    assert ref.sample_counts([0, 5, 5, 12, 13], 0.3).tolist() == [2, 0, 3, 1]
    assert ref.sample_counts([0, 10, 20], np.array([0.5, 1.0])).tolist() == [5, 10]
    # the product is rounded to fp32 before the ceiling, as the device forms it: 10 * fp32(0.3) = 3 + 2^-23 exactly, a tie
    # that rounds to 3.0 (the exact product's ceiling would be 4)
    assert ref.sample_counts([0, 10], 0.3).tolist() == [3]


@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def test_fps_argument_validation(lib):
    """Every check fails before any device work: NULL pointers all the way."""
    rc = lib.dmet_fps_f32(None, None, 1, 10, 0, None, None, 5, None, None, 0, None)
    assert rc == -22 and b"D=0" in lib.dmet_last_error()
    rc = lib.dmet_fps_f32(None, None, 1, 10, 65, None, None, 5, None, None, 0, None)
    assert rc == -22 and b"D=65" in lib.dmet_last_error()
    rc = lib.dmet_fps_f32(None, None, 1, -1, 3, None, None, 5, None, None, 0, None)
    assert rc == -22 and b"N=-1" in lib.dmet_last_error()
    rc = lib.dmet_fps_f32(None, None, -2, 10, 3, None, None, 5, None, None, 0, None)
    assert rc == -22 and b"B=-2" in lib.dmet_last_error()
    rc = lib.dmet_fps_f32(None, None, 1, 10, 3, None, None, -5, None, None, 0, None)
    assert rc == -22 and b"M=-5" in lib.dmet_last_error()
    need = lib.dmet_fps_workspace_bytes(10, 1, 3)
    assert need > 0
    rc = lib.dmet_fps_f32(None, None, 1, 10, 3, None, None, 5, None, None, need - 1, None)
    assert rc == -22 and b"ws_bytes" in lib.dmet_last_error()
    rc = lib.dmet_fps_f32(None, None, 1, 10, 3, None, None, 5, None, None, need, None)
    assert rc == -22 and b"x is NULL" in lib.dmet_last_error()


def test_fps_empty_problems_and_workspace(lib):
    assert lib.dmet_fps_f32(None, None, 0, 10, 3, None, None, 5, None, None, 0, None) == 0
    assert lib.dmet_fps_f32(None, None, 1, 0, 3, None, None, 5, None, None, 0, None) == 0
    assert lib.dmet_fps_f32(None, None, 1, 10, 3, None, None, 0, None, None, 0, None) == 0
    assert lib.dmet_fps_workspace_bytes(0, 1, 3) == 0
    sizes = [lib.dmet_fps_workspace_bytes(n, 4, 3) for n in (1, 2, 1000, 36864, 36865, 10 ** 6, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0


def test_native_constants_match_the_header():
    from deepmetv2_amd import _native
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dmet.h")).read()
    assert f"#define DMET_FPS_THREADS {_native.FPS_THREADS} " in text
    assert f"#define DMET_FPS_LDS_FLOATS {_native.FPS_LDS_FLOATS} " in text
    assert "#define DMET_FPS_LDS_NODES(D) (DMET_FPS_LDS_FLOATS / ((D) + 1))" in text
    assert _native.FPS_LDS_NODES(3) == _native.FPS_LDS_FLOATS // 4
    assert _native.FPS_LDS_NODES(64) * 65 <= _native.FPS_LDS_FLOATS < (_native.FPS_LDS_NODES(64) + 1) * 65


def test_python_errors_before_any_native_call(monkeypatch):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native

    def never(*a, **k):
        raise AssertionError("_native was reached")
    monkeypatch.setattr(_native, "fps", never)
    monkeypatch.setattr(_native, "knn_xy", never)
    x = torch.randn(10, 3)
    for bad in (0, 0.0, 1.5, float("nan"), -0.25, True, "half"):
        with pytest.raises(ValueError, match="ratio must be a float in"):
            dm.fps(x, ratio=bad)
    with pytest.raises(ValueError, match="tensor ratio"):
        dm.fps(x, ratio=torch.tensor([1, 2]))
    with pytest.raises(TypeError, match="ptr must be a 1-D int64"):
        dm.fps(x, ptr=torch.tensor([0, 10], dtype=torch.int32))
    with pytest.raises(TypeError, match="ptr must be a 1-D int64"):
        dm.fps(x, ptr=[0, 10])
    with pytest.raises(ValueError, match=r"x must be \[N, D\]"):
        dm.fps(torch.randn(2, 5, 3))
    with pytest.raises(TypeError, match="float32"):
        dm.fps(x.double())
    with pytest.raises(RuntimeError, match="not on a GPU"):
        dm.fps(x, ratio=0.5)
    with pytest.raises(RuntimeError, match="not on a GPU"):
        dm.fps(x, ptr=torch.tensor([0, 10]), random_start=False)
    with pytest.raises(ValueError, match="coordinates"):
        dm.nearest(x, torch.randn(4, 2))
    with pytest.raises(ValueError, match="given together"):
        dm.nearest(x, torch.randn(4, 3), batch_x=torch.zeros(10, dtype=torch.long))

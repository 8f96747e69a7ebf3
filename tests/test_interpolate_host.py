"""knn_interpolate without a GPU: the float64 reference against a plain triple loop, gradcheck and the upstream formula
from positions; the argument errors (raised from shapes, before any device is asked for); -EINVAL through the library."""
import os
import shutil

import pytest
import torch

import interpolate_reference as ir

# 7 targets over 7 sources, k = 4: a full row, rows with -1 at the end / in the middle / at the front, an empty row, a
# repeated source (the NBR7 of test_gravnet_host.py)
NBR7 = torch.tensor([[0, 1, 2, 3],
                     [1, 0, -1, -1],
                     [2, -1, 4, 6],
                     [-1, 3, 5, -1],
                     [-1, -1, -1, -1],
                     [5, 5, 0, 6],
                     [6, 2, 1, 0]], dtype=torch.int32)


def _inputs7(F=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(7, F, generator=g, dtype=torch.float64)
    dist = torch.rand(7, 4, generator=g).pow(3) * 4.0          # fp32, three decades
    dist[0, 1] = 0.0                                           # a coincident point: clamped to 1e-16
    dist[NBR7 < 0] = 1e10                                      # what the build leaves in an empty slot ...
    dist[3, 0] = 0.25                                          # ... and a value that must be ignored just the same
    return x, dist


def _loops(x, nbr, dist):
    Nt, k = nbr.shape
    Ns, F = x.shape
    out = [[0.0] * F for _ in range(Nt)]
    bar = [[0.0] * F for _ in range(Nt)]
    W = [0.0] * Nt
    for i in range(Nt):
        slots = [t for t in range(k) if 0 <= int(nbr[i, t]) < Ns]
        w = {t: 1.0 / max(float(dist[i, t]), ir.MIN_D) for t in slots}
        W[i] = sum(w[t] for t in slots)
        for t in slots:
            j = int(nbr[i, t])
            for f in range(F):
                out[i][f] += w[t] / W[i] * float(x[j, f])
                bar[i][f] += w[t] / W[i] * abs(float(x[j, f]))
    return (torch.tensor(out, dtype=torch.float64), torch.tensor(bar, dtype=torch.float64),
            torch.tensor(W, dtype=torch.float64))


def test_reference_equals_the_triple_loop():
    x, dist = _inputs7()
    out, bar, W, valid = ir.interpolate(x, NBR7, dist)
    l_out, l_bar, l_W = _loops(x, NBR7, dist)
    torch.testing.assert_close(out, l_out, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(bar, l_bar, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(W, l_W, rtol=1e-13, atol=0)
    assert torch.equal(valid, NBR7 >= 0)
    assert torch.equal(out[4], torch.zeros(5, dtype=torch.float64)) and float(W[4]) == 0.0
    # row 0 holds a coincident point: its weight 1e16 takes the whole row
    torch.testing.assert_close(out[0], x[1], rtol=0, atol=1e-5)
    # an id outside the sources is an empty slot too
    nbr = NBR7.clone()
    nbr[6, 1] = 7
    out2, _bar, _W, valid2 = ir.interpolate(x, nbr, dist)
    assert not bool(valid2[6, 1])
    torch.testing.assert_close(out2, _loops(x, nbr, dist)[0], rtol=1e-13, atol=1e-15)


def test_reference_gradcheck_and_source_side():
    x, dist = _inputs7(F=3, seed=1)
    x.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: ir.interpolate(a, NBR7, dist)[0], (x,), eps=1e-6, atol=1e-6)
    g = torch.randn(7, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ir.interpolate(x, NBR7, dist)[0].backward(g)
    g_x, bar_g, n = ir.source_side(g, NBR7, dist, 7)
    torch.testing.assert_close(g_x, x.grad, rtol=1e-13, atol=1e-15)
    assert n.tolist() == [4, 3, 3, 2, 1, 3, 3]
    assert bool((bar_g >= g_x.abs() * (1 - 1e-12)).all())
    # no source at all: every slot is empty
    out, bar, W, valid = ir.interpolate(torch.zeros(0, 3, dtype=torch.float64), NBR7, dist)
    assert out.shape == (7, 3) and not bool(valid.any()) and not bool(out.any()) and not bool(W.any())


def test_reference_equals_the_upstream_formula_from_positions():
    """nbr from a float64 brute force over tie-free random positions, dist = the fp32 rounding of the float64 distances:
    rounding d moves w by one unit roundoff (2^-24) and r by two; a factor 2 covers second order."""
    g = torch.Generator().manual_seed(3)
    Ns, Nt, F, k = 23, 61, 6, 3
    pos_x = torch.randn(Ns, 3, generator=g, dtype=torch.float64)
    pos_y = torch.randn(Nt, 3, generator=g, dtype=torch.float64)
    x = torch.randn(Ns, F, generator=g, dtype=torch.float64)
    d2 = (pos_y.unsqueeze(1) - pos_x.unsqueeze(0)).pow(2).sum(-1)
    d_k, nbr = d2.topk(k, dim=1, largest=False)
    # upstream, over the edge list (y_idx, x_idx)
    y_idx = torch.arange(Nt).repeat_interleave(k)
    x_idx = nbr.reshape(-1)
    diff = pos_x[x_idx] - pos_y[y_idx]
    w = 1.0 / torch.clamp((diff * diff).sum(-1, keepdim=True), min=1e-16)
    up = torch.zeros(Nt, F, dtype=torch.float64).index_add_(0, y_idx, x[x_idx] * w) / \
        torch.zeros(Nt, 1, dtype=torch.float64).index_add_(0, y_idx, w)
    out, bar, W, valid = ir.interpolate(x, nbr.to(torch.int32), d_k.float())
    assert bool(valid.all())
    err = (out - up).abs()
    print("max err / bar:", float((err / bar).max()), "limit", 4 * 2.0 ** -24)
    assert bool((err <= 4 * 2.0 ** -24 * bar).all())
    torch.testing.assert_close(W, torch.zeros(Nt, 1, dtype=torch.float64).index_add_(0, y_idx, w).view(-1), rtol=2.0 ** -23,
                               atol=0)


def _xy_table(nbr, dist, num_candidates, cnt=None):
    import deepmetv2_amd as dm
    return dm.BipartiteTable(nbr, torch.tensor([0, num_candidates]), torch.tensor([0, nbr.shape[0]]), num_candidates,
                             dist=dist, cnt=cnt)


def test_check_shapes_argument_errors():
    from deepmetv2_amd import _native
    x, dist = torch.randn(7, 5), torch.rand(7, 4)
    _native.interpolate_check_shapes(x, NBR7, dist)
    _native.interpolate_check_shapes(torch.randn(7, 256), torch.zeros(7, 64, dtype=torch.int32), torch.rand(7, 64))
    with pytest.raises(ValueError, match="2-D"):
        _native.interpolate_check_shapes(x[0], NBR7, dist)
    with pytest.raises(ValueError, match="F=257"):
        _native.interpolate_check_shapes(torch.randn(7, 257), NBR7, dist)
    with pytest.raises(ValueError, match="F=0"):
        _native.interpolate_check_shapes(torch.randn(7, 0), NBR7, dist)
    with pytest.raises(ValueError, match="k=65"):
        _native.interpolate_check_shapes(x, torch.zeros(7, 65, dtype=torch.int32), torch.rand(7, 65))
    with pytest.raises(ValueError, match="k=0"):
        _native.interpolate_check_shapes(x, torch.zeros(7, 0, dtype=torch.int32), torch.rand(7, 0))
    with pytest.raises(ValueError, match="distances"):
        _native.interpolate_check_shapes(x, NBR7, torch.rand(7, 3))
    with pytest.raises(ValueError, match="do not fit"):
        _native.interpolate_bwd(torch.randn(7, 5), dist, torch.rand(6), torch.zeros(8, dtype=torch.int32),
                                torch.zeros(28, dtype=torch.int32), 7)
    # well-formed arguments get as far as the device check: there is no CPU implementation
    with pytest.raises(RuntimeError, match="non-GPU"):
        _native.interpolate_fwd(x, NBR7, dist)
    with pytest.raises(RuntimeError, match="non-GPU"):
        _native.interpolate_bwd(torch.randn(7, 5), dist, torch.rand(7), torch.zeros(8, dtype=torch.int32),
                                torch.zeros(28, dtype=torch.int32), 7)


def test_aggregate_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    x, dist = torch.randn(7, 5), torch.rand(7, 4)
    table = _xy_table(NBR7, dist, 7)
    with pytest.raises(ValueError, match="counted"):
        dm.interpolate_aggregate(x, _xy_table(NBR7, dist, 7, cnt=torch.full((7,), 4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="distances"):
        dm.interpolate_aggregate(x, _xy_table(NBR7, None, 7))
    with pytest.raises(ValueError, match="candidates"):
        dm.interpolate_aggregate(x[:6], table)
    with pytest.raises(ValueError, match="F=257"):
        dm.interpolate_aggregate(torch.randn(7, 257), table)
    with pytest.raises(ValueError, match="k=65"):
        dm.interpolate_aggregate(x, _xy_table(torch.zeros(7, 65, dtype=torch.int32), torch.rand(7, 65), 7))
    with pytest.raises(TypeError, match="table must be"):
        dm.interpolate_aggregate(x, NBR7)
    with pytest.raises(TypeError, match="float32"):
        dm.interpolate_aggregate(x.double(), table)
    with pytest.raises(TypeError, match="float32"):
        dm.interpolate_aggregate(x.half(), table)               # fp16 outside fp16 autocast stays an error
    # one node set: a NeighborTable, with the same refusals
    one = dm.NeighborTable(NBR7, torch.tensor([0, 7]), dense=False, dist=dist)
    with pytest.raises(ValueError, match="counted"):
        dm.interpolate_aggregate(x, dm.NeighborTable(NBR7, torch.tensor([0, 7]), dense=False, dist=dist,
                                                     cnt=torch.full((7,), 4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="distances"):
        dm.interpolate_aggregate(x, dm.NeighborTable(NBR7, torch.tensor([0, 7]), dense=False))
    with pytest.raises(ValueError, match="candidates"):
        dm.interpolate_aggregate(torch.randn(8, 5), one)
    for t in (table, one):
        with pytest.raises(RuntimeError, match="non-GPU"):
            dm.interpolate_aggregate(x, t)


def test_knn_interpolate_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    x, pos_x, pos_y = torch.randn(7, 5), torch.randn(7, 3), torch.randn(20, 3)
    bx, by = torch.zeros(7, dtype=torch.long), torch.zeros(20, dtype=torch.long)
    with pytest.raises(ValueError, match="rows"):
        dm.knn_interpolate(x[:6], pos_x, pos_y)
    with pytest.raises(ValueError, match="F in 1..256"):
        dm.knn_interpolate(torch.randn(7, 257), pos_x, pos_y)
    with pytest.raises(ValueError, match="positive int"):
        dm.knn_interpolate(x, pos_x, pos_y, k=0)
    with pytest.raises(ValueError, match="k=65"):
        dm.knn_interpolate(x, pos_x, pos_y, k=65)
    with pytest.raises(ValueError, match="coordinates"):
        dm.knn_interpolate(x, pos_x, torch.randn(20, 2))
    with pytest.raises(ValueError, match="together"):
        dm.knn_interpolate(x, pos_x, pos_y, bx)
    with pytest.raises(ValueError):
        dm.knn_interpolate(x, pos_x, pos_y, period=[None, -1.0, None])
    with pytest.raises(RuntimeError, match="non-GPU"):
        dm.knn_interpolate(x, pos_x, pos_y, bx, by, k=3, num_workers=4)


@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def test_einval_through_the_library(lib):
    """Bad arguments come back as -EINVAL with a message, before any device work (the pointers are never touched)."""
    p = 64      # any non-null address
    for k, F, Nt, word in ((0, 8, 10, b"k=0"), (65, 8, 10, b"k=65"), (3, 0, 10, b"F=0"), (3, 257, 10, b"F=257"),
                           (3, 8, -1, b"Nt=-1")):
        assert lib.dmet_interpolate_fwd_f32(p, p, p, Nt, 5, k, F, p, p, None) == -22
        assert word in lib.dmet_last_error() and b"dmet_interpolate_fwd_f32" in lib.dmet_last_error()
        assert lib.dmet_interpolate_bwd_f32(p, p, p, p, p, Nt, 5, k, F, p, None) == -22
        assert word in lib.dmet_last_error() and b"dmet_interpolate_bwd_f32" in lib.dmet_last_error()
    assert lib.dmet_interpolate_fwd_f32(p, p, p, 10, -2, 3, 8, p, p, None) == -22
    # null pointers
    assert lib.dmet_interpolate_fwd_f32(p, None, p, 10, 5, 3, 8, p, p, None) == -22
    assert b"null" in lib.dmet_last_error()
    assert lib.dmet_interpolate_fwd_f32(None, p, p, 10, 5, 3, 8, p, p, None) == -22
    assert lib.dmet_interpolate_fwd_f32(p, p, p, 10, 5, 3, 8, p, None, None) == -22
    assert lib.dmet_interpolate_bwd_f32(p, p, p, p, p, 10, 5, 3, 8, None, None) == -22
    assert lib.dmet_interpolate_bwd_f32(p, p, None, p, p, 10, 5, 3, 8, p, None) == -22
    assert b"null" in lib.dmet_last_error()
    # empty problems are no-ops: no target in the forward, no source in the backward
    assert lib.dmet_interpolate_fwd_f32(None, None, None, 0, 5, 3, 8, None, None, None) == 0
    assert lib.dmet_interpolate_bwd_f32(None, None, None, None, None, 10, 0, 3, 8, None, None) == 0


def test_names_are_exported():
    import deepmetv2_amd as dm
    assert "knn_interpolate" in dm.__all__ and "interpolate_aggregate" in dm.__all__
    assert callable(dm.knn_interpolate) and callable(dm.interpolate_aggregate)
    assert "knn_interpolate" in dm.__doc__

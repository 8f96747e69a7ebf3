"""The two carriers of the BatchNorm transform that are otherwise checked only at workload-like sizes or through the whole
model -- the node-level dense layer (dmet_bn_node_linear_split_f32) and the kNN prep launch (dmet_bn_knn_local_dense_f32)
-- at the edges of their 32-row tiles.  Every comparison is exact: the reference is _native.bn_apply on the same operands
(the kernel whose functions the carriers call, csrc/bn_affine.h), which test_gpu_parity.py holds to a float64 BatchNorm.
"""
import functools
import os

import pytest
import torch

import per_node_reference as pn

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1       # torch.nn.BatchNorm1d's defaults
# a wavefront owns 32-row tiles: one partial tile, one row short of a tile, one row over, two tiles plus one row
NLS_N = [1, 31, 33, 65]
# the prep kernel's 32-row tiles per event, an empty event, a query-tile boundary
KNN_SIZES = [1, 31, 33, 0, 129]


def _equal(a, b, what):
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} against {tuple(b.shape)}"
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ in their bits"


@functools.lru_cache(maxsize=None)
def _rows(N):
    """CPU inputs of one case: (raw, residual, BatchNorm state, W [32, 64], b [32])."""
    raw, res, _ = pn.bn_rows(N, 32, seed=N + 7)
    g = torch.Generator().manual_seed(N)
    return raw, res, pn.bn_state(32, seed=5), torch.randn(32, 64, generator=g) * 0.2, torch.randn(32, generator=g)


def _operands(dev, N, with_res):
    """Device operands of the transform, statistics from bn_stats: (raw, residual or None, gamma, beta, mean, invstd, W, b)."""
    from deepmetv2_amd import _native
    raw, res, state, W, b = _rows(N)
    raw_d = raw.to(dev)
    mean, invstd = _native.bn_stats(raw_d, EPS, MOMENTUM, state["running_mean"].to(dev), state["running_var"].to(dev))
    return (raw_d, res.to(dev) if with_res else None, state["weight"].to(dev), state["bias"].to(dev), mean, invstd,
            W.to(dev), b.to(dev))


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("N", NLS_N)
def test_bn_node_linear_split_has_the_bits_of_the_two_steps(dev, N, with_res, sliced):
    """_native.bn_node_linear_split on aligned operands: y = bn_apply(...), (P, Q) = node_linear_split(y, W, b, sliced)."""
    from deepmetv2_amd import _native
    *affine, W, b = _operands(dev, N, with_res)
    out = _native.bn_node_linear_split(*affine, W, b, sliced)
    assert out is not None, "bn_node_linear_split declined aligned 32 -> 32 operands"
    y, P, Q = out
    _equal(y, _native.bn_apply(*affine), "y")
    P0, Q0 = _native.node_linear_split(y, W, b, sliced)
    _equal(P, P0, "P")
    _equal(Q, Q0, "Q")


@pytest.mark.parametrize("with_res", [False, True])
def test_bn_knn_local_dense_has_the_bits_of_the_two_steps(dev, with_res):
    """_native.bn_knn_local_dense without a dense request: y = bn_apply(...), (nbr, dist, loc) = knn_local(y, ptr, 16)."""
    from deepmetv2_amd import _native
    *affine, _, _ = _operands(dev, sum(KNN_SIZES), with_res)
    ptr = torch.tensor([0] + KNN_SIZES, dtype=torch.int64).cumsum(0).to(dev)
    out = _native.bn_knn_local_dense(*affine, ptr, 16)
    if os.environ.get("DMET_KNN_PATH") == "exact":
        # by design: the exact kernel has no prep launch for the transform to ride in, the entry launches nothing
        assert out is None
        return
    assert out is not None, "a 32-feature build with k <= 20 takes the matrix-core path"
    y, nbr, dist, loc, pq = out
    assert pq is None
    _equal(y, _native.bn_apply(*affine), "y")
    nbr0, dist0, loc0 = _native.knn_local(y, ptr, 16)
    _equal(nbr, nbr0, "nbr")
    _equal(dist, dist0, "dist")
    _equal(loc, loc0, "loc")

"""Voxel clustering without a GPU: the reference formulas against hand-written examples, the argument refusals that
fire before any device work (CPU tensors never reach a kernel), and the exports."""
import pytest
import torch

from voxel_reference import (MAX_CELLS, cells_of, coarsen_ref, consecutive_cluster_ref, cut_nvox, grid_cluster_ref, grid_spec,
                             nvox_of, voxel_grid_ref)


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def test_reference_1d_boundary_and_end():
    # nvox = trunc(3 / 1) + 1 = 4; 1.0 lies exactly on a boundary and belongs to the upper cell; 3.0 = end is cell 3
    pos = torch.tensor([0.0, 0.5, 1.0, 1.999, 2.0, 3.0])
    want = torch.tensor([0, 0, 1, 1, 2, 3])
    assert nvox_of(*grid_spec(pos, 1.0, 0.0, 3.0)) == [4]
    assert torch.equal(grid_cluster_ref(pos, 1.0, 0.0, 3.0), want)
    assert torch.equal(grid_cluster_ref(pos, 1.0, 0.0, 3.0, clamp=False), want)
    assert torch.equal(grid_cluster_ref(pos, 1.0), want)                # start / end = min / max: the same grid


def test_reference_2d_per_dimension_size():
    # nvox = (trunc(2 / 1) + 1, trunc(1 / 0.5) + 1) = (3, 3); id = c0 + 3 c1
    pos = torch.tensor([[0.0, 0.0], [1.5, 0.2], [2.0, 1.0], [0.4, 0.5], [1.0, 0.49]])
    want = torch.tensor([0, 1, 2 + 3 * 2, 0 + 3 * 1, 1])
    assert nvox_of(*grid_spec(pos, (1.0, 0.5), (0.0, 0.0), (2.0, 1.0))) == [3, 3]
    assert torch.equal(grid_cluster_ref(pos, (1.0, 0.5), (0.0, 0.0), (2.0, 1.0)), want)
    assert torch.equal(grid_cluster_ref(pos, (1.0, 0.5), (0.0, 0.0), (2.0, 1.0), clamp=False), want)


def test_reference_3d_two_events():
    # nvox = (2, 2, 3): 12 cells per event, the event is the most significant digit
    pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 2.0], [0.5, 1.5, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 2.5]])
    batch = torch.tensor([0, 0, 0, 1, 1])
    local = torch.tensor([0, 1 + 2 + 4 * 2, 0 + 2 + 4, 1, 0 + 2 + 4 * 2])
    assert cells_of(pos, 1.0, 0.0, (1.0, 1.0, 2.5)) == 12
    assert torch.equal(grid_cluster_ref(pos, 1.0, 0.0, (1.0, 1.0, 2.5)), local)
    assert torch.equal(voxel_grid_ref(pos, 1.0, batch, 0.0, (1.0, 1.0, 2.5)), local + 12 * batch)


def test_reference_one_cell_and_clamp_rule():
    pos = torch.tensor([[0.1, 0.2], [0.9, 0.8], [0.5, 0.5]])
    assert torch.equal(grid_cluster_ref(pos, 5.0), torch.zeros(3, dtype=torch.int64))          # one cell
    assert torch.equal(voxel_grid_ref(pos, 5.0, torch.tensor([0, 1, 1])), torch.tensor([0, 1, 1]))
    # outside [start, end] and non-finite: clamped per dimension, NaN to cell 0
    stray = torch.tensor([-7.0, 0.0, 2.5, 99.0, float("nan"), float("inf"), float("-inf")])
    assert torch.equal(grid_cluster_ref(stray, 1.0, 0.0, 3.0), torch.tensor([0, 0, 2, 3, 0, 3, 0]))
    # a non-finite or negative (end - start) / size is one cell
    assert nvox_of(*grid_spec(stray, 1.0, 3.0, 0.0)) == [1]
    assert nvox_of(*grid_spec(stray, 1.0, 0.0, float("inf"))) == [1]
    assert nvox_of(*grid_spec(stray, 1.0)) == [1]                       # min / max of a vector with a NaN
    assert cut_nvox([2 ** 20, 2 ** 20, 7]) == [2 ** 20, 4095, 1] and 2 ** 20 * 4095 <= MAX_CELLS


def test_reference_coarsening():
    cluster = torch.tensor([7, 3, 7, 12, 3, 40, 41])
    batch = torch.tensor([0, 0, 0, 0, 0, 2, 2])
    node_map, perm = consecutive_cluster_ref(cluster)
    assert node_map.tolist() == [1, 0, 1, 2, 0, 3, 4] and perm.tolist() == [4, 2, 3, 5, 6]     # the highest index
    co = coarsen_ref(cluster, batch, 4)
    assert co["order"].tolist() == [1, 4, 0, 2, 3, 5, 6] and co["rowptr"].tolist() == [0, 2, 4, 5, 6, 7]
    assert co["C"] == 5 and co["batch"].tolist() == [0, 0, 0, 2, 2] and co["ptr"].tolist() == [0, 3, 3, 5, 5]
    assert (co["max_nodes"], co["min_nodes"]) == (3, 0)


# ---------------------------------------------------------------------------------------------------------------
# refusals before any device work
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["grid_cluster", "voxel_grid"])
def op(request):
    import deepmetv2_amd as dm
    fn = getattr(dm, request.param)
    if request.param == "voxel_grid":
        return lambda pos, size, start=None, end=None: fn(pos, size, None, start, end)
    return fn


def test_exports():
    import deepmetv2_amd as dm
    for name in ("grid_cluster", "voxel_grid", "consecutive_cluster"):
        assert callable(getattr(dm, name)) and name in dm.__all__ and name in dm.__doc__


@pytest.mark.parametrize("D", [0, 9])
def test_refuses_dimension(op, D):
    with pytest.raises(ValueError, match="1 <= D <= 8"):
        op(torch.zeros(4, D), 1.0)
    with pytest.raises(ValueError, match="1 <= D <= 8"):
        op(torch.zeros(4, 2, 2), 1.0)


def test_refuses_float64_and_integers(op):
    with pytest.raises(TypeError, match="float64"):
        op(torch.zeros(4, 2, dtype=torch.float64), 1.0)
    with pytest.raises(TypeError, match="int64"):
        op(torch.zeros(4, 2, dtype=torch.int64), 1.0)


@pytest.mark.parametrize("size", [0.0, -1.0, float("nan"), float("inf"), (1.0, 0.0), (1.0, float("nan")), 1e-50,
                                  torch.tensor([1.0, -2.0])])
def test_refuses_size(op, size):
    with pytest.raises(ValueError, match="size must be positive and finite"):
        op(torch.zeros(4, 2), size, 0.0, 1.0)


@pytest.mark.parametrize("kw", [dict(size=(1.0, 1.0, 1.0)), dict(size=1.0, start=(0.0, 0.0, 0.0)), dict(size=1.0, end=(1.0,) * 5),
                                dict(size=torch.ones(3)), dict(size=1.0, start=torch.zeros(2, 2)), dict(size=())])
def test_refuses_wrong_lengths(op, kw):
    with pytest.raises(ValueError, match="one per dimension"):
        op(torch.zeros(4, 2), **kw)


def test_refuses_host_known_overflow(op):
    pos = torch.zeros(4, 2)
    with pytest.raises(ValueError, match=r"more than 2\^32 - 1"):
        op(pos, 1.0, 0.0, 1e6)                              # (10^6 + 1)^2 cells
    with pytest.raises(ValueError, match=r"more than 2\^32 - 1"):
        op(pos, (1e-3, 1.0), (0.0, 0.0), (1e7, 0.0))        # one dimension alone: 10^10 + 1
    with pytest.raises(ValueError, match=r"more than 2\^32 - 1"):
        op(pos, 1e-20, 0.0, 1e15)                           # a finite fp32 quotient far beyond any integer type


def test_valid_arguments_reach_the_device_check(op):
    """Arguments that pass every refusal above end at the package's own "non-GPU tensor" error: nothing ran."""
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        op(torch.zeros(4, 2), (1.0, 0.5), 0.0, (65535.0, 32767.0))      # 65536 * 65535 cells: the most that fits
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        op(torch.zeros(4), 1.0)

"""The three fused edge-MLP routes at the smallest shape where what their kernels share can go wrong: two workgroups, one
target's and one source's run of edges across a tile edge of both tile geometries, nodes without edges at both ends.
Each route is held to the checks and tolerances of its own test file."""
import pytest
import torch

from edge_mlp_reference import kernel_winners, max64, ref64
from test_gpu_edge_mlp_bf16 import _check as _check_bf16
from test_gpu_edge_mlp_f16 import _check as _check_f16
from test_gpu_edge_mlp_f32 import _close as _close_f32, _conv as _conv_f32, _count_fused, _mlp, _run

pytestmark = pytest.mark.gpu

N, E, HIN, H1, H2 = 40, 2051, 16, 32, 32      # E > 2048: edge_blocks(E) = 2 workgroups
TILE = 2048 // H2                             # 64 edges: the fp32 tile, and the second edge of the 32-edge matrix-core tile


def _graph(dev):
    """[2, E] source -> target.  Nodes 0 and N - 1 have no edge.  In- and out-degrees are the same sequence: node 1 has 50
    and node 2 has 40, so that grouped by target as by source node 2's run is positions 50 .. 89, across TILE."""
    deg = torch.zeros(N, dtype=torch.int64)
    deg[1], deg[2] = 50, 40
    rest = E - 90
    deg[3:N - 1] = rest // (N - 4)
    deg[3] += rest - int(deg[3:N - 1].sum())
    assert int(deg.sum()) == E and deg[0] == 0 and deg[N - 1] == 0 and int(deg[1]) < TILE < int(deg[1] + deg[2])
    tgt = torch.repeat_interleave(torch.arange(N), deg)
    src = tgt[torch.randperm(E, generator=torch.Generator().manual_seed(3))]
    return torch.stack([src, tgt]).to(dev)


CASES = [(aggr, bn) for aggr in ("max", "add", "mean") for bn in (None, "train")]


@pytest.mark.parametrize("route", ["f32", "bf16", "f16"])
def test_runs_across_tile_and_workgroup_edges(dev, monkeypatch, route):
    ei = _graph(dev)
    x = torch.randn(N, HIN, generator=torch.Generator().manual_seed(1)).to(dev)
    for aggr, bn in CASES:
        nn = _mlp(HIN, H1, H2, bn=bn, seed=2)
        if route == "bf16":
            out, gx, _grads, _bufs = _check_bf16(dev, nn, x, ei, aggr, monkeypatch=monkeypatch)
        elif route == "f16":
            out, gx, _grads, _bufs = _check_f16(dev, nn, x, ei, aggr, monkeypatch=monkeypatch)
        else:
            calls = _count_fused(monkeypatch)
            out, gx, grads, _bufs, g = _run(_conv_f32(nn, dev, aggr=aggr), x, ei)
            assert len(calls) == 1
            if aggr == "max":
                # the forward against a maximum that takes nothing from the kernel; its winners serve the gradients alone
                grouped, win = kernel_winners(nn, x, ei, "source_to_target", "f32")
                _r_out, r_gx, r_grads = ref64(nn, x, grouped, aggr, "source_to_target", g, win)
                ref = (max64(nn, x, ei, "source_to_target"), r_gx, r_grads)
            else:
                ref = ref64(nn, x, ei, aggr, "source_to_target", g)
            _close_f32((out, gx, grads), ref, (aggr, bn))
        # R3: the nodes without an edge give 0 and take no gradient
        assert not bool(out[0].any()) and not bool(out[N - 1].any()), (aggr, bn)
        assert not bool(gx[0].any()) and not bool(gx[N - 1].any()), (aggr, bn)

"""The two-set EdgeConv / DynamicEdgeConv on the GPU (generic route over dmet_edge_features_xy_f32): the edge-feature
kernel bit for bit, forward and backward against the same module in float64 over the reference table's edges, with the
bars of the generic-route comparisons in tests/test_gpu_short_rows.py (1e-4 of the largest reference magnitude for the
output and the input gradients, per layer for the parameter gradients)."""
import numpy as np
import pytest
import torch

import knn_xy_reference as xy
from test_knn_xy_host import _nn, check_against_float64

pytestmark = pytest.mark.gpu

SX = [300, 0, 70, 5, 1, 40]         # sources (candidates) per event
SY = [150, 30, 0, 64, 1, 200]       # destinations (queries) per event: event 1 has no source -> rows without an edge


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _batch(sizes, dev):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)


@pytest.mark.parametrize("H", [32, 8, 3, 130])
def test_edge_features_kernel_bit_exact(dev, H):
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(H)
    Ns, Nd, E = 211, 97, 5000
    xs, xd = torch.randn(Ns, H, generator=g).to(dev), torch.randn(Nd, H, generator=g).to(dev)
    src = torch.randint(0, Ns, (E,), generator=g).int().to(dev)
    tgt = torch.randint(0, Nd, (E,), generator=g).int().sort().values.to(dev)
    feat = _native.edge_features_xy(xs, xd, src, tgt)
    want = torch.cat([xd[tgt.long()], xs[src.long()] - xd[tgt.long()]], 1)
    assert torch.equal(feat, want)
    # backward: g_x_dst over the rows, g_x_src over the by-source grouping, against float64 sums
    from deepmetv2_amd.graph import EdgeList
    rowptr = torch.zeros(Nd + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = torch.bincount(tgt.long(), minlength=Nd).cumsum(0).int()
    edges = EdgeList(src, tgt, rowptr, Nd, num_src=Ns)
    srcptr, srcperm = edges.by_source()
    gf = torch.randn(E, 2 * H, generator=g).to(dev)
    g_src, g_dst = _native.edge_features_xy_bwd(gf, rowptr, srcptr, srcperm, Ns, Nd, H)
    g_src2, g_dst2 = _native.edge_features_xy_bwd(gf, rowptr, srcptr, srcperm, Ns, Nd, H)
    assert torch.equal(g_src, g_src2) and torch.equal(g_dst, g_dst2)            # the same bits run to run
    r_dst = torch.zeros(Nd, H, dtype=torch.float64, device=dev).index_add_(0, tgt.long(), (gf[:, :H] - gf[:, H:]).double())
    r_src = torch.zeros(Ns, H, dtype=torch.float64, device=dev).index_add_(0, src.long(), gf[:, H:].double())
    torch.testing.assert_close(g_dst.double(), r_dst, rtol=1e-5, atol=1e-5 * float(r_dst.abs().max()))
    torch.testing.assert_close(g_src.double(), r_src, rtol=1e-5, atol=1e-5 * float(r_src.abs().max()))
    only_dst = _native.edge_features_xy_bwd(gf, rowptr, srcptr, srcperm, Ns, Nd, H, want_src=False)
    assert only_dst[0] is None and torch.equal(only_dst[1], g_dst)


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
@pytest.mark.parametrize("kind", ["linear", "mlp_bn"])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_two_set_edgeconv(dev, aggr, kind, flow):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(21)
    F, H, k = 32, 16, 8
    pos_s, pos_d = torch.randn(sum(SX), 3, generator=g), torch.randn(sum(SY), 3, generator=g)
    x_src, x_dst = torch.randn(sum(SX), F, generator=g), torch.randn(sum(SY), F, generator=g)
    e = xy.edges_of(xy.knn_table(pos_s.numpy(), _ptr(SX), pos_d.numpy(), _ptr(SY), k)[0])
    tgt, src = torch.from_numpy(e[0]), torch.from_numpy(e[1])
    assert int(torch.bincount(tgt, minlength=sum(SY)).min()) == 0                # destination rows with no edge
    assert int(torch.bincount(src, minlength=sum(SX)).min()) == 0                # source rows no edge leaves
    ei = dm.knn(pos_s.to(dev), pos_d.to(dev), k, _batch(SX, dev), _batch(SY, dev), batch_size=len(SX))   # [dst, src]
    assert torch.equal(ei.cpu(), torch.stack([tgt, src]))
    if flow == "source_to_target":
        ei = ei.flip(0)
    conv = dm.EdgeConv(_nn(kind, F, H), aggr=aggr, flow=flow).to(dev).train()
    out, _ref = check_against_float64(conv, lambda xs, xd: conv((xs, xd), ei), x_src.to(dev), x_dst.to(dev), src, tgt,
                                      aggr, torch.randn(sum(SY), H, generator=g).to(dev))
    empty = torch.bincount(tgt, minlength=sum(SY)) == 0
    assert bool((out.cpu()[empty] == 0).all())


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
@pytest.mark.parametrize("kind", ["linear", "mlp_bn"])
def test_two_set_dynamic_edgeconv(dev, aggr, kind):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(22)
    F, H, k = 8, 16, 8
    x_src, x_dst = torch.randn(sum(SX), F, generator=g), torch.randn(sum(SY), F, generator=g)
    e = xy.edges_of(xy.knn_table(x_src.numpy(), _ptr(SX), x_dst.numpy(), _ptr(SY), k)[0])
    tgt, src = torch.from_numpy(e[0]), torch.from_numpy(e[1])
    conv = dm.DynamicEdgeConv(_nn(kind, F, H), k=k, aggr=aggr).to(dev).train()
    bx, by = _batch(SX + [0], dev), _batch(SY + [7], dev)          # a trailing query event that x does not contain
    x_dst = torch.cat([x_dst, torch.randn(7, F, generator=g)])
    out, _ref = check_against_float64(conv, lambda xs, xd: conv((xs, xd), (bx, by)), x_src.to(dev), x_dst.to(dev), src,
                                      tgt, aggr, torch.randn(sum(SY) + 7, H, generator=g).to(dev))
    assert bool((out[-7:] == 0).all()) and bool((out[150:180] == 0).all())


def test_range_checks_on_the_device(dev):
    import deepmetv2_amd as dm
    conv = dm.EdgeConv(_nn("linear", 4, 3)).to(dev)
    xs, xd = torch.randn(5, 4, device=dev), torch.randn(3, 4, device=dev)
    with pytest.raises(ValueError, match="source ids"):
        conv((xs, xd), torch.tensor([[5], [0]], device=dev))
    with pytest.raises(ValueError, match="target ids"):
        conv((xs, xd), torch.tensor([[4], [3]], device=dev))
    assert conv((xs, xd), torch.tensor([[4, 0], [2, 2]], device=dev)).shape == (3, 3)

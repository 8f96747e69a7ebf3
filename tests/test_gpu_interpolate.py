"""knn_interpolate on the GPU (csrc/interpolate.hip, deepmetv2_amd/interpolate.py) against the float64 reference of
tests/interpolate_reference.py over the same table and the table's own fp32 distances.

Bars, per element, with u = 2^-23 and bar = sum_t r_t |x[j_t, f]| (the reference's):
  out   |out - ref| <= (2k + 8) u bar + 1e-30.  First order: one rounding in w, at most k in W, two in r, at most k in the
        fma chain, (2k + 2) unit roundoffs of bar; the rest is margin for a divide that is not correctly rounded and for
        second order.
  wsum  relative error <= (k + 2) u.
  g_x   |g_x - ref| <= (k + n_j + 8) u bar_g, n_j the length of source j's list, bar_g = sum_p r_p |g_out[i_p, f]|.
A simulation of these chains on the CPU (k in 1..64, distances with zeros, equal values and 30 decades, a non-fused fp32
chain) stays at or below a quarter of each limit.  Every row and every element is checked.
"""
import ctypes
import math

import pytest
import torch

import interpolate_reference as ir

pytestmark = pytest.mark.gpu

U = 2.0 ** -23


def _ragged(sizes, dev):
    counts = torch.tensor(sizes, dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return batch.to(dev), int(counts.sum())


def _cloud(fine, coarse, F, seed, dev, D=3):
    """(x[Nc, F], pos_c[Nc, D], pos_f[Nf, D], batch_c, batch_f) on the device: random positions, random coarse features."""
    g = torch.Generator().manual_seed(seed)
    bf, Nf = _ragged(fine, dev)
    bc, Nc = _ragged(coarse, dev)
    x = torch.randn(Nc, F, generator=g)
    pos_c = torch.randn(Nc, D, generator=g)
    pos_f = torch.randn(Nf, D, generator=g)
    return x.to(dev), pos_c.to(dev), pos_f.to(dev), bc, bf


def _table(pos_c, pos_f, k, bc, bf, B, period=None):
    import deepmetv2_amd as dm
    return dm.knn_xy_table(pos_c, pos_f, k, bc, bf, batch_size=B, period=period)


def _run(x, table, g=None):
    """GPU forward + backward: (out, wsum, g_x, g)."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    xx = x.detach().requires_grad_(True)        # shares x's storage: an unaligned view stays one
    out = dm.interpolate_aggregate(xx, table)
    if g is None:
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    raw, wsum = _native.interpolate_fwd(x.detach().float(), table.nbr, table.dist)
    assert torch.equal(raw.to(out.dtype), out.detach())
    return out.detach(), wsum, xx.grad, g


def _check(x, table, what=""):
    """Output, wsum and g_x of interpolate_aggregate against the float64 reference on (table.nbr, table.dist).  Returns
    (out, wsum, g_x, valid, n) with valid and n (the sources' list lengths) from the reference."""
    out, wsum, g_x, g = _run(x, table)
    nbr, dist = table.nbr.cpu(), table.dist.cpu()
    Ns, k = x.shape[0], nbr.shape[1]
    x64 = x.detach().cpu().double()
    r_out, bar, W, valid = ir.interpolate(x64, nbr, dist)
    got = out.cpu().double()
    assert got.shape == r_out.shape and bool(torch.isfinite(got).all()), what
    err, lim = (got - r_out).abs(), (2 * k + 8) * U * bar + 1e-30
    if err.numel():
        print(f"{what}: out max err/limit {float((err / lim).max()):.3f}")
    assert bool((err <= lim).all()), (what, "out", float((err / lim).max()))
    ws = wsum.cpu().double()
    assert ws.shape == W.shape and bool(torch.isfinite(ws).all()), what
    assert bool(((ws - W).abs() <= (k + 2) * U * W).all()), (what, "wsum")
    # rows without a valid slot: exact zeros and wsum 0
    empty = ~valid.any(1)
    assert bool((got[empty] == 0).all()) and bool((ws[empty] == 0).all()), what
    assert bool((ws[~empty] > 0).all()), what
    # backward
    r_gx, bar_g, n = ir.source_side(g.cpu().double(), nbr, dist, Ns)
    gx = g_x.cpu().double()
    assert gx.shape == r_gx.shape and bool(torch.isfinite(gx).all()), what
    gerr, glim = (gx - r_gx).abs(), (k + n.double().unsqueeze(-1) + 8) * U * bar_g
    if gerr.numel() and bool((glim > 0).any()):
        print(f"{what}: g_x max err/limit {float((gerr[glim > 0] / glim[glim > 0]).max()):.3f}")
    assert bool((gerr <= glim).all()), (what, "g_x")
    assert bool((gx[n == 0] == 0).all()), what         # a source nobody lists
    return out, wsum, g_x, valid, n


# ---- 1. shapes ----------------------------------------------------------------------------------------------------------
# the kernels give a row to 16, 32 or 64 lanes by F and by whether rows are read as float4 (F % 4 == 0) or float by float,
# take slots in chunks of that many lanes and gather 4 rows at a time
CASES = {
    "smallest": ([1], [1], 1, 1),
    "upstream default": ([40, 7], [10, 2], 64, 3),
    "empty events": ([5, 0, 9], [3, 4, 0], 22, 3),
    "limits": ([70, 3], [70, 64], 256, 64),
    "several workgroups": ([300, 129, 7, 9], [75, 33, 2, 3], 64, 3),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cases(dev, case):
    fine, coarse, F, k = CASES[case]
    x, pos_c, pos_f, bc, bf = _cloud(fine, coarse, F, len(case), dev)
    table = _table(pos_c, pos_f, k, bc, bf, len(fine))
    out, wsum, g_x, valid, n = _check(x, table, what=case)
    assert out.shape == (sum(fine), F) and g_x.shape == x.shape
    if case == "upstream default":
        assert bool(valid[:40].all()) and bool((valid[40:].sum(1) == 2).all())       # the second event has short rows
    if case == "empty events":
        assert bool(valid[:5].all()) and not bool(valid[5:].any())
        assert bool((out[5:] == 0).all()) and bool((wsum[5:] == 0).all())             # event 2: no coarse node
        assert n[3:7].tolist() == [0, 0, 0, 0] and bool((g_x[3:7] == 0).all())        # event 1: no fine node
    if case == "limits":
        assert bool(valid.all())


@pytest.mark.parametrize("F", [3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256])
def test_channel_sweep(dev, F):
    x, pos_c, pos_f, bc, bf = _cloud([19], [6], F, 100 + F, dev)
    _check(x, _table(pos_c, pos_f, 3, bc, bf, 1), what=f"F={F}")


@pytest.mark.parametrize("k", [1, 2, 4, 15, 16, 17, 31, 32, 33, 63, 64])
def test_slot_sweep(dev, k):
    x, pos_c, pos_f, bc, bf = _cloud([21], [70], 8, 200 + k, dev)
    _out, _wsum, _gx, valid, _n = _check(x, _table(pos_c, pos_f, k, bc, bf, 1), what=f"k={k}")
    assert bool(valid.all())


def test_hub(dev):
    """600 fine nodes, 5 centres, three of them near every fine node: lists of 600 entries, each walked by one group."""
    g = torch.Generator().manual_seed(7)
    pos_f = 0.1 * torch.randn(600, 3, generator=g)
    pos_c = torch.cat([0.1 * torch.randn(3, 3, generator=g), 50.0 + torch.randn(2, 3, generator=g)])
    x = torch.randn(5, 22, generator=g)
    import deepmetv2_amd as dm
    table = dm.knn_xy_table(pos_c.to(dev), pos_f.to(dev), 3)
    _out, _wsum, _gx, valid, n = _check(x.to(dev), table, what="hub")
    assert n.tolist() == [600, 600, 600, 0, 0] and bool(valid.all())


# ---- 2. properties ------------------------------------------------------------------------------------------------------
def test_k1_is_a_gather_of_the_nearest(dev):
    import deepmetv2_amd as dm
    fine, coarse, F = [40, 7, 33], [10, 2, 9], 22
    x, pos_c, pos_f, bc, bf = _cloud(fine, coarse, F, 8, dev)
    xx = x.clone().requires_grad_(True)
    out = dm.knn_interpolate(xx, pos_c, pos_f, bc, bf, k=1)
    idx = dm.nearest(pos_f, pos_c, bf, bc)
    assert torch.equal(out.detach(), x[idx])                    # r = w / w = 1 and fmaf(1, x, 0) = x: bit for bit
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    out.backward(g)
    g64, i64 = g.cpu().double(), idx.cpu()
    ref = torch.zeros(x.shape, dtype=torch.float64).index_add_(0, i64, g64)
    bar_g = torch.zeros(x.shape, dtype=torch.float64).index_add_(0, i64, g64.abs())
    n = torch.bincount(i64, minlength=x.shape[0]).double().unsqueeze(-1)
    assert bool(((xx.grad.cpu().double() - ref).abs() <= (1 + n + 8) * U * bar_g).all())


def test_coincident_points(dev):
    """pos_y holds copies of rows of pos_x: d = 0 exactly, w = 1e16, and nothing overflows."""
    x, pos_c, pos_f, bc, bf = _cloud([30, 12], [8, 5], 22, 10, dev)
    pos_f[0:4] = pos_c[0:4]
    pos_f[30:33] = pos_c[8:11]
    pos_f[4] = pos_c[0]                                         # two fine nodes on the same centre
    table = _table(pos_c, pos_f, 3, bc, bf, 2)
    on = torch.tensor([0, 1, 2, 3, 4, 30, 31, 32], device=dev)
    assert bool((table.dist[on, 0] == 0).all())
    out, wsum, g_x, _valid, _n = _check(x, table, what="coincident")
    assert bool((wsum[on] >= 9e15).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(g_x).all())
    torch.testing.assert_close(out[on], x[table.nbr[on, 0].long()], rtol=0, atol=1e-6)


def test_one_set_table_with_blanked_slots(dev):
    """knn_table(..., loop=False) searches k + 1 and blanks the node itself: a -1 in a slot whose dist is 0, not the
    sentinel.  The validity mask comes from nbr, never from dist."""
    import deepmetv2_amd as dm
    batch, N = _ragged([40, 3, 17], dev)
    g = torch.Generator().manual_seed(11)
    pos, x = torch.randn(N, 3, generator=g).to(dev), torch.randn(N, 22, generator=g).to(dev)
    table = dm.knn_table(pos, 4, batch, loop=False)
    assert isinstance(table, dm.NeighborTable) and table.nbr.shape == (N, 5)
    blank = table.nbr < 0
    assert bool(blank.any(1).all()) and bool((table.dist[blank] == 0).any())
    _out, _wsum, _gx, valid, _n = _check(x, table, what="one set")
    assert torch.equal(valid, ~blank.cpu())


def test_period_wraps_phi(dev):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(12)
    pos_c = torch.tensor([[0.0, 3.1], [0.0, -1.0]])             # (eta, phi): one centre across the seam, one not
    pos_f = torch.stack([0.1 * torch.randn(9, generator=g), torch.full((9,), -3.1)], 1)
    x = torch.randn(2, 22, generator=g)
    per = [None, 2 * math.pi]
    table = dm.knn_xy_table(pos_c.to(dev), pos_f.to(dev), 2, period=per)
    assert bool((table.nbr[:, 0] == 0).all()) and bool((table.dist[:, 0] < 0.2).all())      # 2 pi - 6.2 = 0.083
    _check(x.to(dev), table, what="period")
    wrapped = dm.knn_interpolate(x.to(dev), pos_c.to(dev), pos_f.to(dev), k=2, period=per)
    plain = dm.knn_interpolate(x.to(dev), pos_c.to(dev), pos_f.to(dev), k=2)
    assert torch.equal(wrapped, dm.interpolate_aggregate(x.to(dev), table))
    assert not torch.equal(wrapped, plain)
    # across the seam the first centre takes nearly all the weight; without the period the second one does
    assert bool(((wrapped - x[0].to(dev)).abs().amax(1) < (plain - x[0].to(dev)).abs().amax(1)).all())


def test_unaligned_view_gives_the_same_bits(dev):
    from deepmetv2_amd import _native
    x, pos_c, pos_f, bc, bf = _cloud([40, 7], [10, 2], 64, 13, dev)
    table = _table(pos_c, pos_f, 3, bc, bf, 2)
    flat = torch.zeros(x.numel() + 1, device=dev)
    view = flat[1:].view_as(x)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and x.data_ptr() % 16 == 0
    a, b = _run(x, table), _run(view, table)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # the backward's g_out as such a view
    g = a[3]
    gflat = torch.zeros(g.numel() + 1, device=dev)
    gview = gflat[1:].view_as(g)
    gview.copy_(g)
    assert gview.data_ptr() % 16 == 4
    rev_ptr, rev_pos = table.reverse()
    g_x = _native.interpolate_bwd(gview, table.dist, a[1], rev_ptr, rev_pos, x.shape[0])
    assert torch.equal(g_x, a[2])


def test_bf16(dev):
    import deepmetv2_amd as dm
    x, pos_c, pos_f, bc, bf = _cloud([40, 7], [10, 2], 64, 14, dev)
    table = _table(pos_c, pos_f, 3, bc, bf, 2)
    xb = x.to(torch.bfloat16)
    out = dm.interpolate_aggregate(xb, table)
    full = dm.interpolate_aggregate(xb.float(), table)
    assert out.dtype == torch.bfloat16 and full.dtype == torch.float32 and torch.equal(out, full.to(torch.bfloat16))
    xx = xb.clone().requires_grad_(True)
    dm.interpolate_aggregate(xx, table).float().sum().backward()
    assert xx.grad.dtype == torch.bfloat16 and bool(torch.isfinite(xx.grad.float()).all())
    with pytest.raises(TypeError):
        dm.interpolate_aggregate(x.half(), table)               # fp16 outside fp16 autocast stays an error
    with torch.autocast("cuda", dtype=torch.float16):
        h = dm.interpolate_aggregate(x.half(), table)
    assert h.dtype == torch.float16 and torch.equal(h, dm.interpolate_aggregate(x.half().float(), table).half())


def test_two_runs_give_identical_bits(dev):
    x, pos_c, pos_f, bc, bf = _cloud([300, 129, 7, 9], [75, 33, 2, 3], 64, 15, dev)
    table = _table(pos_c, pos_f, 3, bc, bf, 4)
    a, b = _run(x, table), _run(x, table)
    for p, q in zip(a[:3], b[:3]):
        assert torch.equal(p, q)


def test_knn_interpolate_is_the_aggregate_over_the_xy_table(dev):
    import deepmetv2_amd as dm
    x, pos_c, pos_f, bc, bf = _cloud([40, 7, 0, 12], [10, 2, 5, 3], 22, 16, dev)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    a = dm.knn_interpolate(xa, pos_c, pos_f, bc, bf, k=3, num_workers=8, batch_size=4)
    b = dm.interpolate_aggregate(xb, dm.knn_xy_table(pos_c, pos_f, 3, bc, bf, 4))
    assert torch.equal(a, b)
    g = torch.randn(a.shape, generator=torch.Generator().manual_seed(17)).to(dev)
    a.backward(g)
    b.backward(g)
    assert torch.equal(xa.grad, xb.grad)
    # positions that ask for a gradient get none (upstream forms the weights under no_grad)
    pc = pos_c.clone().requires_grad_(True)
    dm.knn_interpolate(xa, pc, pos_f, bc, bf).sum().backward()
    assert pc.grad is None


def test_every_output_element_is_written(dev):
    """The two C entries over outputs pre-filled with NaN, on the "empty events" shape: finite everywhere and the wrapper's
    bits."""
    from deepmetv2_amd import _lib, _native
    fine, coarse, F, k = CASES["empty events"]
    x, pos_c, pos_f, bc, bf = _cloud(fine, coarse, F, 18, dev)
    table = _table(pos_c, pos_f, k, bc, bf, 3)
    nbr, dist = table.nbr, table.dist
    Nt, Ns = nbr.shape[0], x.shape[0]
    want_out, want_wsum = _native.interpolate_fwd(x, nbr, dist)
    g = torch.randn(Nt, F, generator=torch.Generator().manual_seed(19)).to(dev)
    rev_ptr, rev_pos = table.reverse()
    want_gx = _native.interpolate_bwd(g, dist, want_wsum, rev_ptr, rev_pos, Ns)
    L = _lib.load()
    out = torch.full((Nt, F), float("nan"), device=dev)
    wsum = torch.full((Nt,), float("nan"), device=dev)
    g_x = torch.full((Ns, F), float("nan"), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert L.dmet_interpolate_fwd_f32(x.data_ptr(), nbr.data_ptr(), dist.data_ptr(), Nt, Ns, k, F, out.data_ptr(),
                                      wsum.data_ptr(), stream) == 0
    assert L.dmet_interpolate_bwd_f32(g.data_ptr(), dist.data_ptr(), wsum.data_ptr(), rev_ptr.data_ptr(),
                                      rev_pos.data_ptr(), Nt, Ns, k, F, g_x.data_ptr(), stream) == 0
    torch.cuda.synchronize(dev)
    for got, want in ((out, want_out), (wsum, want_wsum), (g_x, want_gx)):
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    # no target at all: the backward zero-fills g_x
    g_x.fill_(float("nan"))
    assert L.dmet_interpolate_bwd_f32(None, None, None, rev_ptr.data_ptr(), rev_pos.data_ptr(), 0, Ns, k, F,
                                      g_x.data_ptr(), stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((g_x == 0).all())


def test_no_host_sync(dev):
    import deepmetv2_amd as dm
    fine, coarse = [300, 40, 260], [75, 10, 65]
    x, pos_c, pos_f, bc, bf = _cloud(fine, coarse, 64, 20, dev)
    for b, sizes in ((bf, fine), (bc, coarse)):
        ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
        dm.register_batch(b, ptr, 3, max_nodes=max(sizes), min_nodes=min(sizes))
    xx = x.clone().requires_grad_(True)
    dm.knn_interpolate(xx, pos_c, pos_f, bc, bf, k=3).sum().backward()      # module loads, allocator warm-up
    torch.cuda.synchronize()
    g = torch.randn(sum(fine), 64, device=dev)
    xx.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dm.knn_interpolate(xx, pos_c, pos_f, bc, bf, k=3)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(xx.grad).all()) and bool(xx.grad.abs().sum() > 0)


# ---- 3. end to end ------------------------------------------------------------------------------------------------------
def test_down_and_up_chain(dev):
    """fps(ratio=0.25) -> two-set EdgeConv(Linear, 'max') onto the centres -> knn_interpolate back to [N, F] -> Linear(F, 1)
    -> met_reduce, against the same chain in float64 torch built from the GPU's idx and tables.  Gradient bar of
    tests/test_gpu_gravnet.py: rtol 1e-4, atol 1e-4 * max|ref|."""
    import deepmetv2_amd as dm
    sizes, Fin, F, kc = [30, 12], 6, 16, 4
    batch, N = _ragged(sizes, dev)
    g = torch.Generator().manual_seed(21)
    pos, feat, pxy = torch.randn(N, 2, generator=g), torch.randn(N, Fin, generator=g), torch.randn(N, 2, generator=g)
    torch.manual_seed(22)
    lin1, lin2 = torch.nn.Linear(2 * Fin, F).to(dev), torch.nn.Linear(F, 1).to(dev)
    conv = dm.EdgeConv(lin1, aggr="max")
    posd, pxyd = pos.to(dev), pxy.to(dev)
    fx = feat.to(dev).requires_grad_(True)
    idx = dm.fps(posd, batch, 0.25, random_start=False)
    pos_c, batch_c = posd[idx], batch[idx]
    down = dm.knn_xy_table(posd, pos_c, kc, batch, batch_c)               # candidates: fine nodes, queries: centres
    h_c = conv((fx, fx[idx]), down)
    up = dm.knn_xy_table(pos_c, posd, 3, batch_c, batch)
    h_f = dm.knn_interpolate(h_c, pos_c, posd, batch_c, batch, k=3)
    assert torch.equal(h_f, dm.interpolate_aggregate(h_c, up)) and h_f.shape == (N, F)
    met = dm.met_reduce(lin2(h_f).view(-1), pxyd, batch)
    g_met = torch.randn(met.shape, generator=torch.Generator().manual_seed(23)).to(dev)
    met.backward(g_met)

    # the same chain in float64
    i64, b64 = idx.cpu(), batch.cpu()
    assert i64.numel() == 8 + 3                                            # ceil(30 / 4) + ceil(12 / 4)
    W1, b1 = lin1.weight.detach().cpu().double().requires_grad_(True), lin1.bias.detach().cpu().double().requires_grad_(True)
    W2, b2 = lin2.weight.detach().cpu().double().requires_grad_(True), lin2.bias.detach().cpu().double().requires_grad_(True)
    f64 = feat.double().requires_grad_(True)
    dn = down.nbr.cpu().long()
    dvalid = dn >= 0
    assert bool(dvalid.all())
    x_dst = f64[i64].unsqueeze(1).expand(-1, kc, -1)
    msg = torch.cat([x_dst, f64[dn] - x_dst], -1) @ W1.t() + b1            # [M, kc, F]
    r_hc = msg.amax(1)
    r_hf = ir.interpolate(r_hc, up.nbr.cpu(), up.dist.cpu())[0]
    wgt = (r_hf @ W2.t() + b2).view(-1)
    r_met = torch.zeros(len(sizes), 2, dtype=torch.float64).index_add_(0, b64, wgt.unsqueeze(-1) * pxy.double())
    r_met.backward(g_met.cpu().double())
    pairs = [("met", met.detach(), r_met.detach()), ("g_feat", fx.grad, f64.grad), ("g_W1", lin1.weight.grad, W1.grad),
             ("g_b1", lin1.bias.grad, b1.grad), ("g_W2", lin2.weight.grad, W2.grad), ("g_b2", lin2.bias.grad, b2.grad)]
    for name, a, b in pairs:
        scale = max(float(b.abs().max()), 1e-6)
        torch.testing.assert_close(a.cpu().double(), b, rtol=1e-4, atol=1e-4 * scale, msg=lambda m, n=name: f"{n}: {m}")

"""GravNet on the GPU (csrc/gravnet.hip, deepmetv2_amd/gravnet.py) against the float64 reference of
tests/gravnet_reference.py over the same table.

Bars.  Output, per row: |err| <= 1e-5 * bar_i + 1e-6 with bar_i = sum over the valid slots of |h_j|_inf (the form of
tests/test_gpu_edgeconv_linear_sum.py::_check): the weight's error scales with 10 d w <= 1/e, so a message's error is a
few fp32 ulps of |h_j|, not of w |h_j|.  Gradients: rtol 1e-4, atol 1e-4 * max|ref|, that file's bar.  The max may pick
another slot than the reference when two messages differ by less than the output limit, so the reference message at the
GPU's arg is first held to that limit for every (i, p), and the reference backward then routes through the GPU's arg.
The module's output passes two more fp32 Linears; it is held to the gradient bar (rtol 1e-4, atol 1e-4 * max|ref|).
One parameter needs its scale spelt out: lin_s.bias shifts every coordinate alike, the weights see differences only, so
its exact gradient is 0 -- the column sums of g_s over both node sets cancel -- and max|ref| is rounding noise of the
float64 sum (1e-17).  Its atol is 1e-4 * max|ref g_s|, the scale of the terms of that cancelling sum, i.e. the bar g_s
itself is held to; every other parameter keeps max|ref| of its own gradient.
"""
import pytest
import torch

import gravnet_reference as gr

pytestmark = pytest.mark.gpu


def _ragged(sizes, dev):
    counts = torch.tensor(sizes, dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return batch.to(dev), int(counts.sum())


def _data(N, S, P, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, P, generator=g), 0.3 * torch.randn(N, S, generator=g)


def _run(h, s, table, s_dst=None, g=None):
    """GPU forward + backward of the aggregate: (out, arg, g_h, g_s, g_s_dst, g)."""
    from deepmetv2_amd import gravnet
    hh = h.detach().clone().requires_grad_(True)
    ss = s.detach().clone().requires_grad_(True)
    sd = None if s_dst is None else s_dst.detach().clone().requires_grad_(True)
    out, arg = gravnet._aggregate(hh, ss, table, sd)
    if g is None:
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    return out.detach(), arg, hh.grad, ss.grad, None if sd is None else sd.grad, g


def _check(h, s, table, s_dst=None, what=""):
    """Output, max routing and gradients of gravnet_aggregate against the float64 reference on table.nbr."""
    out, arg, g_h, g_s, g_sd, g = _run(h, s, table, s_dst)
    nbr = table.nbr.cpu()
    h64 = h.detach().cpu().double().requires_grad_(True)
    s64 = s.detach().cpu().double().requires_grad_(True)
    sd64 = None if s_dst is None else s_dst.detach().cpu().double().requires_grad_(True)
    r_own, bar, msg, valid, _own = gr.aggregate(h64.detach(), s64.detach(), nbr, None if sd64 is None else sd64.detach())
    P = h.shape[1]
    got = out.cpu().double()
    assert got.shape == r_own.shape and bool(torch.isfinite(got).all()), what
    lim = 1e-5 * bar + 1e-6
    err = (got - r_own).abs().amax(1) if got.numel() else torch.zeros(0, dtype=torch.float64)
    assert bool((err <= lim).all()), (what, "out", float((err - lim).max()))
    # rows without a valid slot: exact zeros and the "no winner" mark
    empty = ~valid.any(1)
    a = arg.cpu().long()
    assert bool((got[empty] == 0).all()) and bool((a[empty] == 255).all()), what
    # the GPU's winner is a valid slot whose reference message lies within the row's limit of the reference maximum
    ne = ~empty
    a_ne = a[ne]
    assert bool((a_ne < nbr.shape[1]).all()), what
    assert bool(valid[ne].gather(1, a_ne)[...].all()) if a_ne.numel() else True, what
    at = msg[ne].gather(1, a_ne.unsqueeze(1)).squeeze(1)
    assert bool((r_own[ne][:, P:] - at <= lim[ne].unsqueeze(1)).all()), (what, "arg")
    # backward: the reference routes its max through the GPU's winners
    r_out = gr.aggregate(h64, s64, nbr, sd64, arg=a)[0]
    r_out.backward(g.cpu().double())
    pairs = [("g_h", g_h, h64.grad), ("g_s", g_s, s64.grad)] + ([("g_s_dst", g_sd, sd64.grad)] if sd64 is not None else [])
    for name, x, ref in pairs:
        x = x.cpu().double()
        assert bool(torch.isfinite(x).all()), (what, name)
        scale = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-6)
        torch.testing.assert_close(x, ref, rtol=1e-4, atol=1e-4 * scale, msg=lambda m, n=name: f"{what}: {n}: {m}")
    return out, arg, g_h, g_s, g_sd, valid


# ---- 1. the aggregate over kNN tables -------------------------------------------------------------------------------------------
# the kernels give a row to 16 lanes (P <= 32, 16 rows per workgroup) or 32 lanes (P > 32, 8 rows per workgroup), take
# slots in chunks of that many and gather 4 rows at a time: sizes sit on both sides of 8, 16, k and the lane count
CASES = {
    "short rows, a one-node and an empty event": ([1, 3, 0, 17, 40], 4, 22, 16),
    "smallest": ([5], 1, 1, 1),
    "limits": ([70, 64], 16, 128, 64),
    "two workgroups and more": ([300, 129, 7, 9, 19, 21, 31, 33], 3, 64, 20),
    "two slot chunks on 16 lanes": ([15, 17, 21, 63, 65], 3, 22, 20),
    "three slot chunks on 16 lanes": ([30, 34, 47], 2, 22, 33),
}


@pytest.mark.parametrize("case", list(CASES))
def test_aggregate_on_knn_tables(dev, case):
    import deepmetv2_amd as dm
    sizes, S, P, k = CASES[case]
    batch, N = _ragged(sizes, dev)
    h, s = _data(N, S, P, seed=len(case))
    table = dm.knn_table(s.to(dev), k, batch, loop=True)
    _out, _arg, _gh, _gs, _gd, valid = _check(h.to(dev), s.to(dev), table, what=case)
    if case == "limits":
        assert bool(valid.all())
    if case.startswith("short rows"):
        assert not bool(valid[:4].all()) and bool(valid[:, 0].all())
    # self is a neighbour at d = 0 exactly (the build's own chain), so w = 1 and the max half is never below h_i itself
    got = dm.gravnet_aggregate(h.to(dev), s.to(dev), table)
    assert bool((got[:, P:] >= h.to(dev)).all())


@pytest.mark.parametrize("P", [15, 16, 17, 32, 33, 64, 65])
def test_every_channel_layout(dev, P):
    """The widths on both sides of the kernels' lane layouts (1 or 2 channels on 16 lanes, 2 or 4 on 32)."""
    import deepmetv2_amd as dm
    batch, N = _ragged([40, 9], dev)
    h, s = _data(N, 4, P, seed=P)
    table = dm.knn_table(s.to(dev), 8, batch, loop=True)
    _check(h.to(dev), s.to(dev), table, what=f"P={P}")


def test_nan_coordinate(dev):
    import deepmetv2_amd as dm
    batch, N = _ragged([12, 30, 9], dev)
    h, s = _data(N, 4, 22, seed=11)
    bad = 12 + 7
    s[bad, 2] = float("nan")
    table = dm.knn_table(s.to(dev), 8, batch, loop=True)
    nbr = table.nbr.cpu()
    assert bool((nbr[bad] == -1).all()) and not bool((nbr == bad).any())
    out, _arg, g_h, g_s, _gd, _valid = _check(h.to(dev), s.to(dev), table, what="nan")
    assert bool((out[bad] == 0).all())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g_h).all()) and bool(torch.isfinite(g_s).all())
    assert bool((g_h[bad] == 0).all()) and bool((g_s[bad] == 0).all())


def test_exact_ties_keep_the_lower_slot(dev):
    import deepmetv2_amd as dm
    h, s = _data(20, 3, 22, seed=12)
    h, s = h.repeat_interleave(2, 0), s.repeat_interleave(2, 0)      # nodes 2m and 2m+1 are identical
    table = dm.knn_table(s.to(dev), 8, None, loop=True)
    nbr = table.nbr.cpu().long()
    assert bool((nbr[:, 0::2] + 1 == nbr[:, 1::2]).all())             # twins sit in slots (0,1), (2,3), ...: R2
    _out, arg, *_ = _check(h.to(dev), s.to(dev), table, what="ties")
    assert bool((arg.cpu() % 2 == 0).all())                            # every max is a tie of twins: the lower slot


def test_underflowed_weights_give_zero_gradients(dev):
    import deepmetv2_amd as dm
    h, s = _data(12, 3, 22, seed=13)
    s[6:, 0] += 5.0                                                     # two clusters of 6, 5 apart: d ~ 25, exp(-250) = 0
    table = dm.knn_table(s.to(dev), 10, None, loop=True)
    far = table.dist > 11.0                                             # expf(-110) is below half the smallest fp32 denormal
    assert int(far.sum()) == 12 * 4 and bool((torch.exp(-10.0 * table.dist[far]) == 0).all())
    _check(h.to(dev), s.to(dev), table, what="underflow")
    # two sets: queries in the first cluster, candidates in both: the far candidates are reached by w == 0 edges only
    q = s[:6] + 0.01
    xy = dm.knn_xy_table(s.to(dev), q.to(dev), 10)
    assert bool((xy.nbr >= 6).sum(1).eq(4).all())
    _out, _arg, g_h, g_s, g_sd, _valid = _check(h.to(dev), s.to(dev), xy, s_dst=q.to(dev), what="underflow xy")
    assert bool((g_h[6:] == 0).all()) and bool((g_s[6:] == 0).all())
    assert bool(g_h[:6].abs().sum() > 0) and bool(torch.isfinite(g_sd).all())


def test_hub_table(dev):
    """A hand-made table: node 0 is in every row, so its reverse row (600 entries) is longer than a workgroup."""
    import deepmetv2_amd as dm
    N, k = 600, 8
    g = torch.Generator().manual_seed(14)
    nbr = torch.randint(0, N, (N, k), generator=g, dtype=torch.int32)
    nbr[torch.rand(N, k, generator=g) < 0.15] = -1
    nbr[:, 0] = 0
    nbr[5, 1:] = -1
    h, s = _data(N, 4, 22, seed=15)
    table = dm.NeighborTable(nbr.to(dev), torch.tensor([0, N], device=dev), dense=False)
    rev_ptr, _pos = table.reverse()
    assert int(rev_ptr[1] - rev_ptr[0]) >= N
    _check(h.to(dev), s.to(dev), table, what="hub")


XY = {
    "an event without candidates": ([40, 0, 50], [12, 9, 16]),
    "an event without queries": ([40, 25, 50], [12, 0, 16]),
}


@pytest.mark.parametrize("case", list(XY))
def test_two_sets(dev, case):
    import deepmetv2_amd as dm
    nx, ny = XY[case]
    bx, Nx = _ragged(nx, dev)
    by, Ny = _ragged(ny, dev)
    h, sx = _data(Nx, 4, 22, seed=16)
    _h, sy = _data(Ny, 4, 22, seed=17)
    table = dm.knn_xy_table(sx.to(dev), sy.to(dev), 8, bx, by, batch_size=3)
    out, *_rest, valid = _check(h.to(dev), sx.to(dev), table, s_dst=sy.to(dev), what=case)
    assert out.shape == (Ny, 44)
    if nx[1] == 0:
        assert not bool(valid[12:21].any()) and bool((out[12:21] == 0).all())
    # the module's pair form against the reference over the same table
    torch.manual_seed(18)
    conv = dm.GravNetConv(10, 12, 4, 22, 8).to(dev)
    g = torch.Generator().manual_seed(19)
    x_l, x_r = torch.randn(Nx, 10, generator=g), torch.randn(Ny, 10, generator=g)
    tab = dm.knn_xy_table(conv.lin_s(x_l.to(dev)).detach(), conv.lin_s(x_r.to(dev)).detach(), 8, bx, by, batch_size=3)
    _module_check(conv, x_l.to(dev), (bx, by), tab, x_r=x_r.to(dev), what=case)


# ---- 2. the module ------------------------------------------------------------------------------------------------------------------
def _ref_of(conv):
    ref = gr.RefGravNetConv(conv.in_channels, conv.out_channels, conv.lin_s.out_features, conv.lin_h.out_features)
    ref.load_state_dict({n: v.detach().cpu().double() for n, v in conv.state_dict().items()})
    return ref


def _module_check(conv, x, batch, table, x_r=None, what=""):
    """Forward, input and parameter gradients of GravNetConv against the float64 reference over `table`."""
    conv.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(True)
    xr = None if x_r is None else x_r.detach().clone().requires_grad_(True)
    out = conv(xx, batch) if xr is None else conv((xx, xr), batch)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(6)).to(out.device)
    out.backward(g)
    ref = _ref_of(conv)
    x64 = x.detach().cpu().double().requires_grad_(True)
    xr64 = None if x_r is None else x_r.detach().cpu().double().requires_grad_(True)
    # route the reference's max through the winners of the GPU aggregate over the same inputs
    from deepmetv2_amd import gravnet
    with torch.no_grad():
        s_l, h_l = conv.lin_s(x), conv.lin_h(x)
        _o, arg = gravnet._aggregate(h_l, s_l, table, None if x_r is None else conv.lin_s(x_r))
    r_out = ref(x64, table.nbr.cpu(), xr64, arg=arg.cpu().long())
    r_out.backward(g.cpu().double())
    got = [("out", out.detach(), r_out.detach()), ("gx", xx.grad, x64.grad)]
    if xr is not None:
        got.append(("gx_r", xr.grad, xr64.grad))
    rp = dict(ref.named_parameters())
    got += [(n, p.grad, rp[n].grad) for n, p in conv.named_parameters()]
    for name, a, b in got:
        scale = max(float(b.abs().max()) if b.numel() else 0.0, 1e-6)
        if name == "lin_s.bias":        # an exactly cancelling sum of g_s rows: the scale of its terms (see the docstring)
            scale = max([scale] + [float(t.grad.abs().max()) for t in ref.coords if t.numel()])
        torch.testing.assert_close(a.cpu().double(), b, rtol=1e-4, atol=1e-4 * scale,
                                   msg=lambda m, n=name: f"{what}: {n}: {m}")
    return out.detach(), xx.grad.detach().clone(), {n: p.grad.detach().clone() for n, p in conv.named_parameters()}


def _module_inputs(dev, sizes=(1, 3, 0, 17, 40, 130), cin=12, seed=20):
    import deepmetv2_amd as dm
    torch.manual_seed(seed)
    conv = dm.GravNetConv(cin, 14, 4, 22, 16).to(dev)
    batch, N = _ragged(list(sizes), dev)
    x = torch.randn(N, cin, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    return conv, x, batch


def test_module_matches_the_reference(dev):
    import deepmetv2_amd as dm
    conv, x, batch = _module_inputs(dev)
    table = dm.knn_table(conv.lin_s(x).detach(), 16, batch, loop=True)
    _module_check(conv, x, batch, table, what="module")
    assert bool((table.nbr[:, 0] == torch.arange(x.shape[0], device=dev)).all())       # self at d = 0, as knn(s, s, k)


def test_module_loads_a_reference_state_dict(dev):
    import deepmetv2_amd as dm
    torch.manual_seed(22)
    ref = gr.RefGravNetConv(12, 14, 4, 22)
    conv = dm.GravNetConv(12, 14, 4, 22, 16)
    conv.load_state_dict({n: v.float() for n, v in ref.state_dict().items()})
    conv = conv.to(dev)
    batch, N = _ragged([50, 23], dev)
    x = torch.randn(N, 12, generator=torch.Generator().manual_seed(23))
    out = conv(x.to(dev), batch)
    table = dm.knn_table(conv.lin_s(x.to(dev)).detach(), 16, batch, loop=True)
    # the parameters were rounded to fp32 once: compare with the reference over those rounded parameters
    r_out = _ref_of(conv)(x.double(), table.nbr.cpu())
    scale = float(r_out.detach().abs().max())
    torch.testing.assert_close(out.detach().cpu().double(), r_out.detach(), rtol=1e-4, atol=1e-4 * scale)
    # and the rounding itself moves the float64 module's output by fp32 epsilons only
    torch.testing.assert_close(r_out.detach(), ref(x.double(), table.nbr.cpu()).detach(), rtol=1e-4, atol=1e-4 * scale)


def test_two_runs_give_identical_bits(dev):
    import deepmetv2_amd as dm
    conv, x, batch = _module_inputs(dev, sizes=(300, 40, 129), seed=24)
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        out = conv(xx, batch)
        out.backward(torch.ones_like(out) * 0.37)
        runs.append([out.detach(), xx.grad] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    h, s = _data(x.shape[0], 4, 22, seed=25)
    table = dm.knn_table(s.to(dev), 16, batch, loop=True)
    r1, r2 = _run(h.to(dev), s.to(dev), table), _run(h.to(dev), s.to(dev), table)
    for a, b in zip(r1[:4], r2[:4]):
        assert torch.equal(a, b)


def test_module_adds_no_host_sync(dev):
    import deepmetv2_amd as dm
    sizes = [300, 40, 260]
    conv, x, batch = _module_inputs(dev, sizes=sizes, seed=26)
    counts = torch.tensor(sizes)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(dev)
    dm.register_batch(batch, ptr, 3, max_nodes=300, min_nodes=40)
    xx = x.clone().requires_grad_(True)
    conv(xx, batch).sum().backward()                    # module loads, allocator warm-up
    torch.cuda.synchronize()
    g = torch.randn(sum(sizes), 14, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = conv(xx, batch)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(xx.grad).all())


def test_bf16_autocast(dev):
    import deepmetv2_amd as dm
    conv, x, batch = _module_inputs(dev, sizes=(60, 33), seed=27)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        s, h = conv.lin_s(x), conv.lin_h(x)
        assert s.dtype == torch.bfloat16 and h.dtype == torch.bfloat16
        table = dm.knn_table(s.detach(), 16, batch, loop=True)
        agg = dm.gravnet_aggregate(h, s, table)
        out = conv(x, batch)
    assert agg.dtype == torch.bfloat16 and out.shape == (x.shape[0], 14)
    full = dm.gravnet_aggregate(h.float(), s.float(), table)
    assert full.dtype == torch.float32 and torch.equal(agg, full.to(torch.bfloat16))
    hh = h.detach().clone().requires_grad_(True)
    ss = s.detach().clone().requires_grad_(True)
    dm.gravnet_aggregate(hh, ss, table).float().sum().backward()
    assert hh.grad.dtype == torch.bfloat16 and ss.grad.dtype == torch.bfloat16 and bool(torch.isfinite(ss.grad.float()).all())
    with pytest.raises(TypeError):
        dm.gravnet_aggregate(h.half(), s.float(), table)           # fp16 outside fp16 autocast stays an error


def _composed(h, s, nbr):
    """The route without the kernels, over a table without empty slots: index_select, exp, index_add, scatter amax."""
    N, k = nbr.shape
    src = nbr.reshape(-1).long()
    tgt = torch.arange(N, device=h.device).repeat_interleave(k)
    w = torch.exp(-10.0 * (s.index_select(0, src) - s.index_select(0, tgt)).pow(2).sum(-1))
    msg = h.index_select(0, src) * w.unsqueeze(-1)
    mean = torch.zeros_like(h).index_add(0, tgt, msg) / k
    mx = torch.full_like(h, float("-inf")).scatter_reduce(0, tgt.unsqueeze(-1).expand_as(msg), msg, "amax")
    return torch.cat([mean, mx], 1)


def test_memory_stays_below_one_message_tensor(dev):
    """8 x 2000 nodes, k 16, P 32, S 4: forward + backward of the aggregate grows the peak by less than one [E, P] fp32
    tensor; the composed route (which also agrees with it) by more."""
    import deepmetv2_amd as dm
    batch, N = _ragged([2000] * 8, dev)
    h, s = _data(N, 4, 32, seed=28)
    h, s = h.to(dev), s.to(dev)
    table = dm.knn_table(s, 16, batch, loop=True)
    table.reverse()
    nbr = table.nbr
    assert bool((nbr >= 0).all())
    one = N * 16 * 32 * 4
    g = torch.randn(N, 64, device=dev)
    grown, outs = {}, {}
    for name, fn in (("fused", lambda a, b: dm.gravnet_aggregate(a, b, table)), ("composed", lambda a, b: _composed(a, b, nbr))):
        hh, ss = h.clone().requires_grad_(True), s.clone().requires_grad_(True)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.max_memory_allocated(dev)
        out = fn(hh, ss)
        out.backward(g)
        torch.cuda.synchronize(dev)
        grown[name] = torch.cuda.max_memory_allocated(dev) - base
        outs[name] = (out.detach(), hh.grad, ss.grad)
        del out
    assert grown["fused"] < one, grown
    assert grown["composed"] > one, grown
    for a, b in zip(outs["fused"], outs["composed"]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))

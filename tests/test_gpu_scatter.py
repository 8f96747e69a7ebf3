"""The reduction layer held to float64: scatter_add / scatter_max (the torch_scatter drop-ins), global_{add,mean,max}_pool,
met_reduce / met_loss / met_loss_from_weights, and what a batch vector's call history may change.

Two kinds of data, so that a kernel that is subtly wrong fails and not only one that is far off:
- exact data: small integers, or multiples of a power of two, chosen so that every partial sum is representable in
  fp32.  Any summation order then gives the exact sum, so sums (and means formed as fp32 sum / fp32 count) must equal
  the float64 reference bit for bit: one dropped, repeated or mis-assigned element fails, even in a 10^6-node segment;
- Gaussian data: each (row, channel) within the rigorous bound of recursive summation in any order,
  |s - s_ref| <= gamma_n * sum |x|, gamma_n = n u / (1 - n u), u = 2^-24, n the segment length.

Every index here lies in [0, n) and every batch value is >= 0: tests/test_scatter_host.py covers the rejected inputs
without a GPU.  NaN inputs of the max reductions are out of scope (the kernel compares with `v > best`, so a NaN
wins only as a row's first entry, and the result then depends on where in the row it sits)."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, g, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64))


def _sum_ref(src, index, n):
    """float64 index_add_ over rows, returned as float64 (exact for exact data)."""
    s = src.double()
    return torch.zeros((n,) + tuple(s.shape[1:]), dtype=torch.float64).index_add_(0, index, s)


def _check_bound(out, src, index, n):
    """|s - s_ref| <= gamma_len * sum|x| per (row, channel), len = the row's segment length."""
    ref = _sum_ref(src, index, n)
    mag = _sum_ref(src.abs(), index, n)
    cnt = torch.bincount(index, minlength=n).double()
    nu = cnt * U
    gamma = (nu / (1 - nu)).view((n,) + (1,) * (src.dim() - 1))
    err = (out.detach().cpu().double() - ref).abs()
    bad = err > gamma * mag
    assert not bool(bad.any()), f"{int(bad.sum())} sums outside the recursive-summation bound, worst err {float(err.max())}"


def _max_ref(src, index, n):
    """(out, arg) of scatter_max in float64 terms: per (row, channel) the lowest position among the entries equal to
    the maximum; out carries that entry's bits (so -0.0 vs +0.0 follows the position), empty rows give 0 and arg = E."""
    E, H = src.shape
    idx = index.view(-1, 1).expand(E, H)
    mx = torch.zeros(n, H).scatter_reduce(0, idx, src, "amax", include_self=False)
    eq = src == mx[index]
    pos = torch.where(eq, torch.arange(E).view(-1, 1).expand(E, H), torch.full((E, H), E))
    arg = torch.full((n, H), E).scatter_reduce(0, idx, pos, "amin", include_self=True)
    out = torch.where(arg < E, src[arg.clamp(max=E - 1), torch.arange(H).view(1, -1)], torch.zeros(n, H))
    return out, arg


# ---------------------------------------------------------------------------------------------------------------
# scatter_add, 1-D (event_sum_kernel through the batch vector; the grouped path for any other index)
# ---------------------------------------------------------------------------------------------------------------
RAGGED_1D = [
    [0, 0, 3, 0, 1, 1024, 1023, 1025, 0, 4096, 4095, 4097, 2, 0, 5],   # empty first / inside; 1024 threads, 4 rows each
    [10 ** 6],
    [1, 4100, 0, 7],
]


def _many_small(g):
    return torch.randint(0, 4, (10 ** 4,), generator=g).tolist()


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_scatter_add_1d_sorted_exact_and_bound(dev, case):
    import deepmetv2_amd as dm
    g = _gen(10 + case)
    sizes = _many_small(g) if case == 3 else RAGGED_1D[case]
    batch = _batch_of(sizes)
    N, B = batch.numel(), len(sizes)
    last = int(batch[-1]) + 1
    src = _ints((N,), g)
    sd = src.to(dev).requires_grad_(True)
    for dim_size in (None, B, B + 3):                  # trailing empty events through dim_size
        bd = batch.to(dev)
        out = dm.scatter_add(sd, bd, dim_size=dim_size)
        n = last if dim_size is None else dim_size
        assert _same_bits(out, _sum_ref(src, batch, n).float())
        assert _same_bits(out, dm.scatter_add(sd, bd, dim_size=dim_size))
    # backward: g[index], exactly
    coef = _ints((B + 3,), g)
    sd.grad = None
    (dm.scatter_add(sd, batch.to(dev), dim_size=B + 3) * coef.to(dev)).sum().backward()
    assert _same_bits(sd.grad, coef[batch])
    # Gaussian data
    gs = torch.randn(N, generator=g)
    out = dm.scatter_add(gs.to(dev), batch.to(dev), dim_size=B)
    _check_bound(out, gs, batch, B)
    assert _same_bits(out, dm.scatter_add(gs.to(dev), batch.to(dev), dim_size=B))


@pytest.mark.parametrize("case", [0, 2, 3])
def test_scatter_add_1d_unsorted(dev, case):
    """An unsorted in-range index gives the reference sums, with and without dim_size, and the same bits again."""
    import deepmetv2_amd as dm
    g = _gen(20 + case)
    sizes = _many_small(g) if case == 3 else RAGGED_1D[case]
    batch = _batch_of(sizes)
    N = batch.numel()
    index = batch[torch.randperm(N, generator=g)]
    last = int(index.max()) + 1
    src = _ints((N,), g)
    for dim_size in (None, len(sizes) + 2):
        n = last if dim_size is None else dim_size
        sd = src.clone().to(dev).requires_grad_(True)
        idx = index.to(dev)
        out = dm.scatter_add(sd, idx, dim_size=dim_size)
        assert _same_bits(out, _sum_ref(src, index, n).float())
        assert _same_bits(out, dm.scatter_add(sd, idx, dim_size=dim_size))
        assert _same_bits(out, dm.scatter_add(sd, index.to(dev), dim_size=dim_size))
        coef = _ints((n,), g)
        (out * coef.to(dev)).sum().backward()
        assert _same_bits(sd.grad, coef[index])
    gs = torch.randn(N, generator=g)
    _check_bound(dm.scatter_add(gs.to(dev), index.to(dev)), gs, index, last)


# ---------------------------------------------------------------------------------------------------------------
# scatter_add, 2-D along dim 0 (reverse-index grouping + segment_reduce_kernel)
# ---------------------------------------------------------------------------------------------------------------
def _patterns(g, E, n):
    srt = torch.sort(torch.randint(0, n, (E,), generator=g)).values
    hub = torch.randint(0, n, (E + 10 ** 5,), generator=g)
    hub[torch.randperm(hub.numel(), generator=g)[:10 ** 5]] = n // 2       # one row receives 10^5 edges
    return {"sorted": (srt, None), "random": (torch.randint(0, n, (E,), generator=g), None),
            "reversed": (torch.flip(srt, [0]), None), "hub": (hub, None),
            "dim_size": (torch.randint(0, n - 7, (E,), generator=g), n + 5)}


def _index_forms(idx, H):
    return {"[E]": idx, "[E,1]": idx.view(-1, 1), "[E,H]": idx.view(-1, 1).expand(-1, H)}


@pytest.mark.parametrize("H", [1, 2, 3, 16, 32, 33, 64, 128, 257])
def test_scatter_add_2d(dev, H):
    import deepmetv2_amd as dm
    g = _gen(100 + H)
    n = 300
    for name, (idx, dim_size) in _patterns(g, 3000, n).items():
        E = idx.numel()
        rows = int(idx.max()) + 1 if dim_size is None else dim_size
        src = _ints((E, H), g)
        ref = _sum_ref(src, idx, rows).float()
        sd = src.to(dev).requires_grad_(True)
        for form, index in _index_forms(idx.to(dev), H).items():
            out = dm.scatter_add(sd, index, dim=0, dim_size=dim_size)
            assert _same_bits(out, ref), (name, form)
        out = dm.scatter_add(sd, idx.to(dev), dim=0, dim_size=dim_size)
        assert _same_bits(out, dm.scatter_add(sd, idx.to(dev), dim=0, dim_size=dim_size))
        coef = _ints((rows, H), g)
        (out * coef.to(dev)).sum().backward()
        assert _same_bits(sd.grad, coef[idx]), name
        gs = torch.randn(E, H, generator=g)
        _check_bound(dm.scatter_add(gs.to(dev), idx.to(dev), dim=0, dim_size=dim_size), gs, idx, rows)


def test_scatter_add_2d_out_and_half(dev):
    import deepmetv2_amd as dm
    g = _gen(7)
    for H in (3, 32, 33):
        idx = torch.randint(0, 50, (4000,), generator=g)
        src = _ints((4000, H), g)
        base = _ints((60, H), g)
        out = base.clone().to(dev)
        res = dm.scatter_add(src.to(dev), idx.to(dev), dim=0, out=out, dim_size=60)
        assert res is out
        assert _same_bits(out, (_sum_ref(src, idx, 60) + base.double()).float())
        out1 = torch.zeros(4000, device=dev)
        s1 = _ints((4000,), g)
        dm.scatter_add(s1.to(dev), idx.to(dev), out=out1[:60], dim_size=60)
        assert _same_bits(out1[:60], _sum_ref(s1, idx, 60).float())
        # bf16 / fp16 src: fp32 sums of the (exact) half values, returned in src.dtype
        for dt in (torch.bfloat16, torch.float16):
            sh = src.to(dt)
            r = dm.scatter_add(sh.to(dev), idx.to(dev), dim=0, dim_size=60)
            assert r.dtype == dt
            assert torch.equal(r.cpu(), _sum_ref(sh.float(), idx, 60).float().to(dt))
            r1 = dm.scatter_add(s1.to(dt).to(dev), torch.sort(idx).values.to(dev), dim_size=60)
            assert r1.dtype == dt
            assert torch.equal(r1.cpu(), _sum_ref(s1.to(dt).float(), torch.sort(idx).values, 60).float().to(dt))
            sg = sh.to(dev).requires_grad_(True)
            coef = _ints((60, H), g)
            (dm.scatter_add(sg, idx.to(dev), dim=0, dim_size=60).float() * coef.to(dev)).sum().backward()
            assert sg.grad.dtype == dt and torch.equal(sg.grad.cpu(), coef[idx].to(dt))


# ---------------------------------------------------------------------------------------------------------------
# scatter_max
# ---------------------------------------------------------------------------------------------------------------
def _check_max(dev, src, idx, dim_size, tag):
    import deepmetv2_amd as dm
    rows = dim_size if dim_size is not None else int(idx.max()) + 1
    E, H = src.shape
    out_ref, arg_ref = _max_ref(src, idx, rows)
    sd = src.clone().to(dev).requires_grad_(True)
    for form, index in _index_forms(idx.to(dev), H).items():
        out, arg = dm.scatter_max(sd, index, dim=0, dim_size=dim_size)
        assert _same_bits(out, out_ref), (tag, form)
        assert torch.equal(arg.cpu(), arg_ref), (tag, form)
    out2, arg2 = dm.scatter_max(sd, idx.to(dev), dim=0, dim_size=dim_size)
    assert _same_bits(out, out2) and torch.equal(arg, arg2)
    coef = _ints((rows, H), g=_gen(E + H))
    (out2 * coef.to(dev)).sum().backward()
    won = arg_ref[idx] == torch.arange(E).view(-1, 1)      # the gradient reaches exactly the arg entries
    assert _same_bits(sd.grad, torch.where(won, coef[idx], torch.zeros(E, H))), tag


@pytest.mark.parametrize("H", [1, 3, 16, 32, 33, 64, 257])
def test_scatter_max_patterns_and_ties(dev, H):
    g = _gen(300 + H)
    for name, (idx, dim_size) in _patterns(g, 3000, 200).items():
        src = _ints((idx.numel(), H), g, -3, 3)             # many exact ties
        _check_max(dev, src, idx, dim_size, name)
    idx, _ = _patterns(g, 3000, 200)["random"]
    _check_max(dev, torch.randn(idx.numel(), H, generator=g), idx, 230, "gaussian")


def test_scatter_max_special_values(dev):
    """All-negative rows (the max is negative, not 0), all -inf rows, +inf entries, -0.0 / +0.0 in one row (the bits of
    the lowest position among the equal values), empty rows (0 and arg = E), the lowest ORIGINAL position on ties when
    the index is unsorted."""
    g = _gen(5)
    E, H, n = 2000, 8, 64
    idx = torch.randint(0, n - 4, (E,), generator=g)          # rows n-4 .. n-1 stay empty
    src = _ints((E, H), g, -3, 3)
    src[idx == 1] = -_ints((int((idx == 1).sum()), H), g, 1, 9)    # all negative
    src[idx == 2] = float("-inf")
    m3 = idx == 3
    src[m3] = _ints((int(m3.sum()), H), g, -2, 2)
    src[torch.nonzero(m3).view(-1)[1], :] = float("inf")
    r4 = torch.nonzero(idx == 4).view(-1)
    src[r4] = -1.0
    src[r4[::2], :4] = -0.0                                   # -0.0 first in columns 0..3 ...
    src[r4[1::2], :4] = 0.0
    src[r4[::2], 4:] = 0.0                                    # ... +0.0 first in columns 4..7
    src[r4[1::2], 4:] = -0.0
    _check_max(dev, src, idx, n, "special")
    import deepmetv2_amd as dm
    out, arg = dm.scatter_max(src.to(dev), idx.to(dev), dim=0, dim_size=n)
    out, arg = out.cpu(), arg.cpu()
    assert bool((out[1] < 0).all()) and bool((out[2] == float("-inf")).all()) and bool((out[3] == float("inf")).all())
    assert torch.equal(torch.signbit(out[4]), torch.tensor([True] * 4 + [False] * 4))
    assert bool((out[n - 4:] == 0).all()) and not bool(torch.signbit(out[n - 4:]).any())
    assert bool((arg[n - 4:] == E).all())
    # unsorted: ties resolved by the lowest original position (the perm remapping), not the grouped one
    perm = torch.randperm(E, generator=g)
    _check_max(dev, src[perm], idx[perm], n, "special, permuted")


def test_scatter_max_half(dev):
    import deepmetv2_amd as dm
    g = _gen(6)
    idx = torch.randint(0, 40, (1500,), generator=g)
    src = torch.randn(1500, 33, generator=g)
    for dt in (torch.bfloat16, torch.float16):
        out_ref, arg_ref = _max_ref(src.to(dt).float(), idx, 40)
        out, arg = dm.scatter_max(src.to(dt).to(dev), idx.to(dev), dim=0, dim_size=40)
        assert out.dtype == dt and torch.equal(out.cpu(), out_ref.to(dt)) and torch.equal(arg.cpu(), arg_ref)


# ---------------------------------------------------------------------------------------------------------------
# global pools (segment_reduce_kernel over the batch vector's ptr)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 32, 64])
def test_global_pools(dev, F):
    import deepmetv2_amd as dm
    g = _gen(400 + F)
    for sizes in ([0, 5, 0, 1, 300, 2, 0], [2 * 10 ** 5], [3, 1]):
        batch = _batch_of(sizes)
        N, B = batch.numel(), len(sizes)
        for size in (None, B + 2):
            rows = int(batch[-1]) + 1 if size is None else size
            x = _ints((N, F), g)
            x[batch == 1] = -_ints((int((batch == 1).sum()), F), g, 1, 8)    # an all-negative event
            xd = x.to(dev).requires_grad_(True)
            bd = batch.to(dev)
            s = _sum_ref(x, batch, rows)
            cnt = torch.bincount(batch, minlength=rows).clamp(min=1).float().view(-1, 1)
            add = dm.global_add_pool(xd, bd, size=size)
            mean = dm.global_mean_pool(xd, bd, size=size)
            mx = dm.global_max_pool(xd, bd, size=size)
            assert _same_bits(add, s.float())
            assert _same_bits(mean, s.float() / cnt)
            out_ref, arg_ref = _max_ref(x, batch, rows)
            assert _same_bits(mx, out_ref)
            for fn, r in ((dm.global_add_pool, add), (dm.global_mean_pool, mean), (dm.global_max_pool, mx)):
                assert _same_bits(fn(xd, bd, size=size), r)
            coef = _ints((rows, F), g)
            (add * coef.to(dev)).sum().backward()
            assert _same_bits(xd.grad, coef[batch])
            xd.grad = None
            (mx * coef.to(dev)).sum().backward()
            won = arg_ref[batch] == torch.arange(N).view(-1, 1)
            assert _same_bits(xd.grad, torch.where(won, coef[batch], torch.zeros(N, F)))
            xd.grad = None
            (mean * 4.0).sum().backward()        # 4 / count: exact for the power-of-two counts, else one rounding
            torch.testing.assert_close(xd.grad.cpu().double(), (4.0 / cnt.double())[batch].expand(N, F), rtol=U, atol=0)
        gs = torch.randn(N, F, generator=g)
        _check_bound(dm.global_add_pool(gs.to(dev), batch.to(dev)), gs, batch, int(batch[-1]) + 1)
    x = _ints((777, F), g)
    xd = x.to(dev)
    assert _same_bits(dm.global_add_pool(xd, None), x.double().sum(0, keepdim=True).float())
    assert _same_bits(dm.global_mean_pool(xd, None), x.double().sum(0, keepdim=True).float() / 777.0)
    assert _same_bits(dm.global_max_pool(xd, None), _max_ref(x, torch.zeros(777, dtype=torch.int64), 1)[0])


# ---------------------------------------------------------------------------------------------------------------
# met_reduce, met_loss, met_loss_from_weights (K4)
# ---------------------------------------------------------------------------------------------------------------
def _met_data(B, g):
    """x [N,11] with px, py multiples of 2^-4 in [-1, 1], w multiples of 2^-8 in [-1/16, 1/16]: every product is a
    multiple of 2^-12 of magnitude <= 1/16, so any partial sum of an event below 65536 nodes is exact in fp32."""
    if B == 1:
        sizes = [5000]
    else:
        sizes = torch.randint(0, 40, (B,), generator=g).tolist()
        sizes[0], sizes[B // 2] = 0, 1500
    batch = _batch_of(sizes)
    N = batch.numel()
    x = torch.randn(N, 11, generator=g)
    x[:, :2] = _ints((N, 2), g, -16, 16) / 16
    w = _ints((N,), g, -16, 16) / 256
    truth = torch.randn(B, 11, generator=g)
    truth[:, :2] = _ints((B, 2), g, -64, 64) / 16
    return x, w, batch, truth


@pytest.mark.parametrize("B", [1, 255, 256, 257, 5000])
def test_met_reduce_and_loss(dev, B):
    import deepmetv2_amd as dm
    from deepmetv2_amd.scatter import met_loss, met_loss_from_weights
    g = _gen(500 + B)
    x, w, batch, truth = _met_data(B, g)
    xd, bd, td = x.to(dev), batch.to(dev), truth.to(dev)
    assert xd.stride(0) == 11
    met_ref = _sum_ref(w.double().view(-1, 1) * x[:, :2].double(), batch, B)
    wd = w.to(dev).requires_grad_(True)
    met = dm.met_reduce(wd, xd, bd, num_events=B)
    assert _same_bits(met, met_ref.float())
    assert _same_bits(met, dm.met_reduce(wd, xd, bd, num_events=B))
    coef = _ints((B, 2), g)
    (met * coef.to(dev)).sum().backward()
    assert _same_bits(wd.grad, (coef[batch, 0].double() * x[:, 0] + coef[batch, 1].double() * x[:, 1]).float())
    # the loss: met is exact, so is met + truth; the rest is squares and a fixed-order sum of 2B non-negative terms
    r = met_ref + truth[:, :2].double()
    loss_ref = 0.5 * (r * r).sum() / B
    g_ref = r / B
    gam = (2 * B + 8) * U
    loss = met_loss(met.detach(), td)
    assert abs(float(loss) - float(loss_ref)) <= gam * float(loss_ref)
    assert _same_bits(loss, met_loss(met.detach(), td))
    for scale in (1.0, 3.7):
        wd.grad = None
        lf = met_loss_from_weights(wd, xd, td, bd)
        assert _same_bits(lf, loss)                        # the fused node gives the chain's bits
        (scale * lf).backward()
        sc = float(torch.tensor(scale, dtype=torch.float32))
        gw_ref = sc * (g_ref[batch, 0] * x[:, 0].double() + g_ref[batch, 1] * x[:, 1].double())
        mag = sc * (g_ref[batch, 0].abs() * x[:, 0].abs().double() + g_ref[batch, 1].abs() * x[:, 1].abs().double())
        err = (wd.grad.cpu().double() - gw_ref).abs()
        assert bool((err <= 8 * U * mag).all()), f"scale {scale}: worst err {float(err.max())}"
        gw1 = wd.grad.clone()
        wd.grad = None
        (scale * met_loss_from_weights(wd, xd, td, bd)).backward()
        assert _same_bits(wd.grad, gw1)
    # the chain met_loss(met_reduce(...)): d loss / d met = r / B per event
    md = met.detach().requires_grad_(True)
    (3.7 * met_loss(md, td)).backward()
    err = (md.grad.cpu().double() - float(torch.tensor(3.7, dtype=torch.float32)) * g_ref).abs()
    assert bool((err <= 4 * U * 3.7 * g_ref.abs()).all())


# ---------------------------------------------------------------------------------------------------------------
# call history: a count one caller passes never changes what another call returns
# ---------------------------------------------------------------------------------------------------------------
def test_call_history(dev):
    import deepmetv2_amd as dm
    g = _gen(9)
    batch = _batch_of([3, 0, 5, 2])           # last event 3: 4 events inferred
    N = batch.numel()
    src = _ints((N,), g).to(dev)
    x = _ints((N, 11), g).to(dev)
    w = _ints((N,), g).to(dev)

    def fresh():
        return batch.to(dev)

    calls = [lambda b, n: dm.scatter_add(src, b, dim_size=n),
             lambda b, n: dm.global_add_pool(x, b, size=n), lambda b, n: dm.global_mean_pool(x, b, size=n),
             lambda b, n: dm.global_max_pool(x, b, size=n), lambda b, n: dm.met_reduce(w, x, b, num_events=n)]
    for call in calls:
        for order in ((None, 7), (7, None), (4, None, 6), (None, 4, 9, None)):
            b = fresh()
            for n in order:
                assert _same_bits(call(b, n), call(fresh(), n)), n
    # unsorted 1-D index, both orders
    idx = batch[torch.randperm(N, generator=g)].to(dev)
    for order in ((None, 6), (6, None)):
        i2 = idx.clone()
        for n in order:
            assert _same_bits(dm.scatter_add(src, i2, dim_size=n), dm.scatter_add(src, idx.clone(), dim_size=n))


# ---------------------------------------------------------------------------------------------------------------
# device -> host syncs
# ---------------------------------------------------------------------------------------------------------------
def _count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    # "called a synchronizing CUDA operation" (HIP on ROCm builds); not the "prototype feature" notice of the mode switch
    return sum("called a synchronizing" in str(r.message) for r in rec)


def test_sync_counts(dev):
    """Validating an unregistered batch shares the reads it always made; a registered batch costs none."""
    import deepmetv2_amd as dm
    g = _gen(11)
    sizes = [4, 0, 9, 3]
    batch = _batch_of(sizes)
    B, N = len(sizes), batch.numel()
    src, x, w = _ints((N,), g).to(dev), _ints((N, 11), g).to(dev), _ints((N,), g).to(dev)
    ptr = torch.tensor([0, 4, 4, 13, 16], device=dev)
    cases = {"scatter_add": (lambda b: dm.scatter_add(src, b), 2),
             "scatter_add dim_size": (lambda b: dm.scatter_add(src, b, dim_size=B), 1),
             "global_add_pool size": (lambda b: dm.global_add_pool(x, b, size=B), 1),
             "met_reduce num_events": (lambda b: dm.met_reduce(w, x, b, num_events=B), 1)}
    for name, (fn, today) in cases.items():
        fn(batch.to(dev))                           # warm-up (library, workspaces)
        b = batch.to(dev)
        n = _count_syncs(lambda: fn(b))
        assert 1 <= n <= today, f"{name}: {n} syncs"
        b = batch.to(dev)
        dm.register_batch(b, ptr, B, max_nodes=9, min_nodes=0)
        assert _count_syncs(lambda: fn(b)) == 0, name

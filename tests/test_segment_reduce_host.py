"""scatter.py's new family (scatter, scatter_mean, scatter_min, scatter_softmax, scatter_log_softmax, scatter_logsumexp,
segment_csr, softmax) and AttentionalAggregation without a GPU, on the CPU stand-ins of tests/segment_reference.py and
tests/fake_native.py: what is refused and when, what delegates to what, and how a grouping is undone."""
import inspect

import pytest
import torch

import deepmetv2_amd as dm
import fake_native
import segment_reference as sr
from deepmetv2_amd import _native

SAFE_FOR_ANY_INPUT = {"batch_to_ptr", "reverse_index"}


@pytest.fixture(autouse=True)
def _fake(monkeypatch):
    fake_native.install(monkeypatch)
    sr.install(monkeypatch)
    monkeypatch.setattr(_native, "_require_device", lambda *t: torch.device("cpu"))


@pytest.fixture
def spy(monkeypatch):
    """Records every `_native` entry called: the public ones and the new `_segment_*` ones."""
    calls = []
    for name, fn in list(vars(_native).items()):
        if not inspect.isfunction(fn) or fn.__module__ not in (_native.__name__, fake_native.__name__, sr.__name__):
            continue
        if name.startswith("_") and name not in sr.NAMES:
            continue

        def wrapped(*a, _name=name, _fn=fn, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        monkeypatch.setattr(_native, name, wrapped)

    class Spy:
        def clear(self):
            calls.clear()

        def unsafe(self):
            return [c for c in calls if c not in SAFE_FOR_ANY_INPUT]

        def names(self):
            return list(calls)
    return Spy()


def _t(v, dtype=torch.int64):
    return torch.tensor(v, dtype=dtype)


FUNCS = {
    "mean": lambda s, i, **kw: dm.scatter_mean(s, i, **kw),
    "min": lambda s, i, **kw: dm.scatter_min(s, i, **kw),
    "softmax": lambda s, i, **kw: dm.scatter_softmax(s, i, **kw),
    "log_softmax": lambda s, i, **kw: dm.scatter_log_softmax(s, i, **kw),
    "logsumexp": lambda s, i, **kw: dm.scatter_logsumexp(s, i, **kw),
    "scatter-mean": lambda s, i, **kw: dm.scatter(s, i, reduce="mean", **kw),
    "scatter-min": lambda s, i, **kw: dm.scatter(s, i, reduce="min", **kw),
}


def test_the_spy_sees_the_new_entries(spy):
    dm.scatter_softmax(torch.randn(4, 2), _t([0, 0, 1, 1]), dim=0)
    dm.scatter_mean(torch.randn(4), _t([0, 0, 1, 1]))
    assert "_segment_softmax_fwd" in spy.names() and "_segment_mean" in spy.names()


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_rejected_inputs_never_reach_a_kernel(spy, name):
    f = FUNCS[name]
    s2, s1 = torch.randn(3, 2), torch.randn(3)
    bad = [
        (TypeError, lambda: f(s2, _t([0, 1, 1], torch.int32), dim=0)),                 # index dtype
        (TypeError, lambda: f(s1, _t([0, 1, 1], torch.int32))),
        (ValueError, lambda: f(s2, _t([0, 1]), dim=0)),                                # shape mismatch
        (ValueError, lambda: f(s1, _t([0, 1]))),
        (ValueError, lambda: f(torch.randn(3, 4), _t([[0, 0], [1, 1], [1, 1]]), dim=0)),
        (IndexError, lambda: f(s2, _t([0, 9, 1]), dim=0, dim_size=4)),                 # outside [0, dim_size)
        (IndexError, lambda: f(s1, _t([0, 4, 1]), dim_size=4)),
        (IndexError, lambda: f(s2, _t([0, 1]).new_tensor([0, 1, 2]), dim=0, dim_size=0)),
        (IndexError, lambda: f(s2, _t([0, -5, 1]), dim=0, dim_size=4)),                # negative
        (IndexError, lambda: f(s2, _t([0, -1, 2]), dim=0)),
        (IndexError, lambda: f(s1, _t([-4, -2, -1]))),
        (NotImplementedError, lambda: f(s2, _t([[0, 1], [1, 0], [1, 1]]), dim=0)),     # per-column indices that differ
        (NotImplementedError, lambda: f(s2, _t([0, 1, 1]), dim=1)),                    # unsupported dim
        (NotImplementedError, lambda: f(s2, _t([0, 1, 1]))),                           # dim=-1 of a 2-D src
        (NotImplementedError, lambda: f(torch.randn(3, 2, 2), _t([0, 1, 1]), dim=0)),
        (TypeError, lambda: f(torch.ones(3, 2, dtype=torch.int64), _t([0, 1, 1]), dim=0)),      # integer src
    ]
    for exc, call in bad:
        spy.clear()
        with pytest.raises(exc):
            call()
        assert spy.unsafe() == [], (exc, spy.unsafe())


def test_scatter_rejects_mul_and_unknown_reduce(spy):
    s, i = torch.randn(3, 2), _t([0, 1, 1])
    with pytest.raises(NotImplementedError, match="mul"):
        dm.scatter(s, i, dim=0, reduce="mul")
    with pytest.raises(ValueError, match="prod"):
        dm.scatter(s, i, dim=0, reduce="prod")
    with pytest.raises(ValueError, match="std"):
        dm.segment_csr(s, _t([0, 1, 3]), reduce="std")
    assert spy.names() == []


def test_scatter_sum_and_max_delegate(spy):
    g = torch.Generator().manual_seed(0)
    src = torch.randint(-8, 9, (40, 3), generator=g).float()
    idx = torch.randint(0, 6, (40,), generator=g)
    for reduce, direct in (("sum", lambda: dm.scatter_add(src, idx, dim=0, dim_size=8)),
                           ("add", lambda: dm.scatter_add(src, idx, dim=0, dim_size=8)),
                           ("max", lambda: dm.scatter_max(src, idx, dim=0, dim_size=8)[0])):
        spy.clear()
        want = direct()
        direct_calls = spy.names()
        spy.clear()
        got = dm.scatter(src, idx, dim=0, dim_size=8, reduce=reduce)
        assert spy.names() == direct_calls and direct_calls
        assert torch.equal(got, want)
    assert dm.scatter_sum is dm.scatter_add
    s1, b = src[:, 0].contiguous(), idx.sort().values
    spy.clear()
    want = dm.scatter_add(s1, b)
    direct_calls = spy.names()
    spy.clear()
    assert torch.equal(dm.scatter(s1, b.clone()), want) and spy.names() == direct_calls       # reduce defaults to 'sum'


def test_the_module_is_callable_as_the_function():
    import deepmetv2_amd.scatter as mod
    assert dm.scatter is mod and callable(dm.scatter) and hasattr(dm.scatter, "met_loss_from_weights")
    for name in ("scatter", "scatter_sum", "scatter_mean", "scatter_min", "scatter_softmax", "scatter_log_softmax",
                 "scatter_logsumexp", "segment_csr", "softmax", "AttentionalAggregation"):
        assert name in dm.__all__ and hasattr(dm, name)


@pytest.mark.parametrize("fn", [dm.scatter_softmax, dm.scatter_log_softmax])
@pytest.mark.parametrize("one_d", [False, True])
def test_unsorted_index_gives_the_sorted_rows_in_src_order(fn, one_d):
    g = torch.Generator().manual_seed(1)
    src = torch.randn(60, generator=g) if one_d else torch.randn(60, 3, generator=g)
    idx = torch.randint(0, 7, (60,), generator=g)
    order = idx.sort(stable=True).indices
    kw = {} if one_d else {"dim": 0}
    sorted_res = fn(src[order].contiguous(), idx[order], dim_size=9, **kw)
    res = fn(src, idx, dim_size=9, **kw)
    assert res.shape == src.shape and torch.equal(res[order], sorted_res)
    rows = src.view(60, -1)
    want = torch.zeros_like(rows)
    for r in range(9):
        sel = idx == r
        if sel.any():
            want[sel] = (torch.softmax if fn is dm.scatter_softmax else torch.log_softmax)(rows[sel].double(), 0).float()
    assert torch.allclose(res.view(60, -1), want, rtol=1e-6, atol=1e-7)


def test_scatter_min_arg_is_a_position_in_the_callers_src():
    g = torch.Generator().manual_seed(2)
    src = torch.randint(-4, 5, (50, 3), generator=g).float()          # many ties
    idx = torch.randint(0, 6, (50,), generator=g)
    idx[idx == 4] = 3                                                 # row 4 is empty, and so are 6 and 7
    out, arg = dm.scatter_min(src, idx, dim=0, dim_size=8)
    assert arg.dtype == torch.int64 and out.shape == (8, 3)
    for r in range(8):
        sel = (idx == r).nonzero().view(-1)
        for c in range(3):
            if sel.numel() == 0:
                assert out[r, c] == 0 and arg[r, c] == 50
            else:
                lowest = sel[(src[sel, c] == src[sel, c].min()).nonzero()[0, 0]]
                assert arg[r, c] == lowest and out[r, c] == src[lowest, c]
    o1, a1 = dm.scatter_min(src[:, 0].contiguous(), idx, dim_size=8)
    assert torch.equal(o1, out[:, 0]) and torch.equal(a1, arg[:, 0])
    assert torch.equal(dm.scatter(src, idx, dim=0, dim_size=8, reduce="min"), out)


def test_backward_goes_back_through_the_grouping():
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 5, (40,), generator=g)
    order = idx.sort(stable=True).indices
    rowptr = sr.lengths_rowptr(torch.bincount(idx, minlength=6).tolist())
    inv = torch.empty_like(order)
    inv[order] = torch.arange(40)
    coef_e, coef_r = torch.randn(40, 3, generator=g), torch.randn(6, 3, generator=g)
    cases = [(dm.scatter_softmax, lambda s: sr.softmax_ref(s[order], rowptr)[inv], coef_e),
             (dm.scatter_log_softmax, lambda s: sr.log_softmax_ref(s[order], rowptr)[inv], coef_e),
             (dm.scatter_logsumexp, lambda s: sr.logsumexp_ref(s[order], rowptr), coef_r),
             (dm.scatter_mean, lambda s: sr.mean_ref(s[order], rowptr), coef_r)]
    for fn, ref, coef in cases:
        src = torch.randn(40, 3, generator=g).requires_grad_(True)
        (fn(src, idx, dim=0, dim_size=6) * coef).sum().backward()
        s64 = src.detach().double().requires_grad_(True)
        (ref(s64) * coef.double()).sum().backward()
        assert torch.allclose(src.grad.double(), s64.grad, rtol=1e-5, atol=1e-6), fn.__name__
    src = torch.randint(-4, 5, (40, 3), generator=g).float().requires_grad_(True)
    out, arg = dm.scatter_min(src, idx, dim=0, dim_size=6)
    (out * coef_r).sum().backward()
    want = torch.zeros(40, 3)
    for r in range(6):
        for c in range(3):
            if arg[r, c] < 40:
                want[arg[r, c], c] = coef_r[r, c]
    assert torch.equal(src.grad, want)


def test_softmax_with_ptr_and_with_a_registered_batch(spy):
    g = torch.Generator().manual_seed(4)
    lengths = [3, 0, 5, 1]
    ptr = sr.lengths_rowptr(lengths).long()
    batch = torch.repeat_interleave(torch.arange(4), torch.tensor(lengths))
    src = torch.randn(9, 2, generator=g)
    want = dm.scatter_softmax(src, batch, dim=0, dim_size=4)
    spy.clear()
    assert torch.equal(dm.softmax(src, ptr=ptr), want)
    assert spy.names() == ["_segment_softmax_fwd"]                    # no grouping: no sort, no read of the index
    other = torch.zeros(9, dtype=torch.int64)
    assert torch.equal(dm.softmax(src, other, ptr=ptr), want)         # ptr wins
    reg = batch.clone()
    dm.register_batch(reg, ptr, 4, max_nodes=5, min_nodes=0)
    spy.clear()
    assert torch.equal(dm.softmax(src, reg), want)
    assert spy.names() == ["_segment_softmax_fwd"]
    assert torch.equal(dm.softmax(src, batch.clone(), num_nodes=4), want)      # any other index is grouped
    assert torch.equal(dm.softmax(src[:, 0].contiguous(), ptr=ptr), want[:, 0])
    assert torch.allclose(dm.softmax(src).sum(0), torch.ones(2))              # neither: one group
    with pytest.raises(NotImplementedError):
        dm.softmax(src, ptr=ptr, dim=1)


def test_segment_csr_matches_the_grouped_scatter(spy):
    g = torch.Generator().manual_seed(5)
    lengths = [2, 0, 4, 1, 0]
    indptr = sr.lengths_rowptr(lengths).long()
    idx = torch.repeat_interleave(torch.arange(5), torch.tensor(lengths))
    src = torch.randint(-8, 9, (7, 3), generator=g).float()
    for reduce in ("sum", "add", "mean", "min", "max"):
        spy.clear()
        got = dm.segment_csr(src, indptr, reduce=reduce)
        assert "reverse_index" not in spy.names()                      # no sort
        assert torch.equal(got, dm.scatter(src, idx, dim=0, dim_size=5, reduce=reduce)), reduce
    assert torch.equal(dm.segment_csr(src[:, 1].contiguous(), indptr, reduce="mean"),
                       dm.scatter_mean(src[:, 1].contiguous(), idx, dim_size=5))
    # a malformed indptr is clamped to [0, E] before any kernel sees it: every span lies inside src or is empty
    rowptrs = []
    real = _native._segment_mean
    try:
        _native._segment_mean = lambda s, rp, ml=0: (rowptrs.append(rp.tolist()), torch.zeros(rp.numel() - 1, s.shape[1]))[1]
        dm.segment_csr(src, _t([-3, 5, 2, 99]), reduce="mean")
    finally:
        _native._segment_mean = real
    assert rowptrs == [[0, 5, 2, 7]]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_src_is_the_fp32_call_rounded_once(dtype):
    g = torch.Generator().manual_seed(6)
    src = torch.randn(30, 3, generator=g).to(dtype)
    idx = torch.randint(0, 4, (30,), generator=g)
    for fn in (dm.scatter_mean, dm.scatter_softmax, dm.scatter_log_softmax, dm.scatter_logsumexp,
               lambda *a, **k: dm.scatter_min(*a, **k)[0]):
        got = fn(src, idx, dim=0, dim_size=5)
        assert got.dtype == dtype and torch.equal(got, fn(src.float(), idx, dim=0, dim_size=5).to(dtype))
    ptr = sr.lengths_rowptr([10, 20]).long()
    assert torch.equal(dm.softmax(src, ptr=ptr), dm.softmax(src.float(), ptr=ptr).to(dtype))
    assert torch.equal(dm.segment_csr(src, ptr, reduce="mean"), dm.segment_csr(src.float(), ptr, reduce="mean").to(dtype))


@pytest.mark.parametrize("gate_out", [1, 4])
def test_attentional_aggregation_is_softmax_times_values_summed(gate_out):
    torch.manual_seed(7)
    lengths = [3, 0, 6, 1]
    ptr = sr.lengths_rowptr(lengths).long()
    batch = torch.repeat_interleave(torch.arange(4), torch.tensor(lengths))
    x = torch.randn(10, 5)
    agg = dm.AttentionalAggregation(torch.nn.Linear(5, gate_out), torch.nn.Linear(5, 4))
    want = torch.zeros(4, 4)
    for b in range(4):
        sel = batch == b
        if sel.any():
            want[b] = (torch.softmax(agg.gate_nn(x[sel]), 0) * agg.nn(x[sel])).sum(0)
    reg = batch.clone()
    dm.register_batch(reg, ptr, 4, max_nodes=6, min_nodes=0)
    for out in (agg(x, ptr=ptr), agg(x, batch, dim_size=4), agg(x, reg)):
        assert out.shape == (4, 4) and torch.allclose(out, want, rtol=1e-5, atol=1e-6)
    agg(x, ptr=ptr).square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in agg.parameters())
    before = agg.nn.weight.detach().clone()
    agg.reset_parameters()
    assert not torch.equal(agg.nn.weight, before)
    plain = dm.AttentionalAggregation(torch.nn.Linear(5, 1))
    assert plain(x, ptr=ptr).shape == (4, 5)
    with pytest.raises(ValueError):
        dm.AttentionalAggregation(torch.nn.Linear(5, 3), torch.nn.Linear(5, 4))(x, ptr=ptr)


def test_eps_is_accepted_and_documented():
    src, idx = torch.randn(6, 2), _t([0, 0, 1, 1, 1, 2])
    assert torch.equal(dm.scatter_log_softmax(src, idx, dim=0, eps=1e-12), dm.scatter_log_softmax(src, idx, dim=0, eps=0.0))
    assert torch.equal(dm.scatter_logsumexp(src, idx, dim=0, eps=1e-12), dm.scatter_logsumexp(src, idx, dim=0, eps=0.0))
    for fn in (dm.scatter_log_softmax, dm.scatter_logsumexp):
        assert "eps" in fn.__doc__ and "rounds to 1" in fn.__doc__

"""The reference the GPU gather-max tests compare with (tests/gather_max_reference.py) is itself checked here, without a
GPU: the vectorised form against a literal triple loop on every input class, and against the oracle's scatter_max (R3, R4)
on the equivalent edge list.  The last test shows that the inputs tell a wrong reference from the right one."""
import numpy as np
import pytest
import torch

from gather_max_reference import VARIANTS, gather_max_loops, gather_max_ref, make_inputs, winner_ids16

SIZES = [0, 1, 17, 140, 0, 33, 70, 0]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("k", [1, 5, 8])
def test_vectorised_reference_is_the_triple_loop(variant, counted, k):
    d = make_inputs(SIZES, k, 8, variant, counted, seed=3)
    out, arg = gather_max_ref(d["P"], d["Q"], d["nbr"], d["cnt"])
    out_l, arg_l = gather_max_loops(d["P"], d["Q"], d["nbr"], d["cnt"])
    assert torch.equal(_bits(out), _bits(out_l)) and torch.equal(arg, arg_l)      # bits: NaN and the sign of zero included


def test_inputs_hold_every_class():
    """What the classes are there for must really occur in the reference's answer."""
    k, H = 8, 8
    d = make_inputs(SIZES, k, H, "finite", False, seed=3)
    out, arg = gather_max_ref(d["P"], d["Q"], d["nbr"])
    nbr, Q = d["nbr"], d["Q"]
    empty = (nbr < 0).all(1)
    assert bool(empty.any()) and bool((out[empty] == 0).all()) and bool((arg[empty] == 255).all())          # (b), R3
    assert bool((nbr[:, 0] < 0)[~empty].any()) and bool((nbr[:, -1] < 0)[~empty].any())                   # holes, both ends
    vals = torch.where((nbr >= 0).unsqueeze(-1), Q[nbr.long().clamp(min=0)], torch.full((), float("-inf")))
    ties = (vals == vals.amax(1, keepdim=True)).sum(1) > 1
    assert bool(ties[:, 2:4].float().mean() > 0.3) and bool(ties[:, 0].any())                               # (c), (a)
    assert bool(torch.isposinf(out).any()) and bool((ties & torch.isposinf(vals.amax(1)))[:, 4:6].any())    # (e)
    tiny = (out != 0) & (out.abs() < 1e-38)
    assert bool(tiny.any())                                                                                 # (d)
    for v, chans in (("g1", [0, 4]), ("g2", [1, 2, 3, 5, 6, 7]), ("g3", list(range(8)))):
        d = make_inputs(SIZES, k, H, v, False, seed=3)
        out, arg = gather_max_ref(d["P"], d["Q"], d["nbr"])
        rows = torch.isneginf(out[:, chans]).all(1)
        others = [c for c in range(H) if c not in chans]
        assert bool(rows.any()) and bool((arg[rows][:, chans] == 255).all())
        assert bool(torch.isfinite(out[rows][:, others]).all()) and bool((arg[rows][:, others] != 255).all())
        assert not bool(torch.isnan(out).any())
    d = make_inputs(SIZES, k, H, "fh", True, seed=3)
    out, arg = gather_max_ref(d["P"], d["Q"], d["nbr"], d["cnt"])
    assert bool(torch.isnan(d["P"]).any()) and not bool(torch.isnan(out).any()) and bool(torch.isneginf(out).any())


@pytest.mark.parametrize("counted", [False, True])
def test_reference_against_the_oracle_scatter_max(counted):
    """R3 / R4 as the oracle states them: the maximum of Q over a row's edges, listed in slot order, the lowest edge
    position winning ties, an empty row giving 0; then the one fp32 add."""
    from oracle import ref_ops
    k, H = 8, 16
    d = make_inputs(SIZES, k, H, "finite", counted, seed=5)
    P, Q, nbr, cnt = d["P"], d["Q"], d["nbr"].long(), d["cnt"]
    N = P.shape[0]
    m = torch.full((N,), k) if cnt is None else cnt.long()
    used = (nbr >= 0) & (torch.arange(k).view(1, -1) < m.view(-1, 1))
    tgt, slot = used.nonzero(as_tuple=True)            # row-major: ascending row, then ascending slot
    src = nbr[tgt, slot]
    best, epos = ref_ops.scatter_max(Q[src], tgt, N)
    some = used.any(1, keepdim=True)
    want_out = torch.where(some, P + best, torch.zeros(()))
    E = src.numel()
    want_arg = torch.where(epos == E, torch.full_like(epos, 255), slot[epos.clamp(max=E - 1)]).to(torch.uint8)
    out, arg = gather_max_ref(P, Q, d["nbr"], cnt)
    assert torch.equal(out, want_out) and torch.equal(arg, want_arg)
    ids = winner_ids16(arg, d["nbr"], d["ptr"])
    lo = torch.repeat_interleave(d["ptr"][:-1], d["ptr"].diff()).view(-1, 1)
    won = torch.where(epos == E, torch.full_like(epos, 0xFFFF), src[epos.clamp(max=E - 1)] - lo)
    assert torch.equal(ids, won)


def test_a_wrong_reference_is_told_apart():
    """Two deliberate breaks of the contract, applied to the reference: ties to the HIGHEST slot, and R3 decided by the
    values of a lane's first channel instead of the ids.  Both must differ from the reference on these inputs -- so a GPU
    form that equals the reference bit for bit cannot equal either of them."""
    k, H = 8, 8
    d = make_inputs(SIZES, k, H, "finite", False, seed=3)
    out, arg = gather_max_ref(d["P"], d["Q"], d["nbr"])
    _, arg_hi = gather_max_ref(d["P"], d["Q"], d["nbr"].flip(1))
    arg_hi = torch.where(arg_hi == 255, arg_hi, (k - 1 - arg_hi.long()).to(torch.uint8))
    assert not torch.equal(arg, arg_hi)
    d = make_inputs(SIZES, k, H, "g1", False, seed=3)
    out, arg = gather_max_ref(d["P"], d["Q"], d["nbr"])
    by_value = (arg.view(-1, H // 4, 4)[:, :, :1] != 255).expand(-1, -1, 4).reshape(-1, H)
    assert not torch.equal(out, torch.where(by_value, out, torch.zeros(())))

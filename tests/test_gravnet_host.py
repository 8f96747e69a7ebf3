"""GravNet without a GPU: the float64 reference against a plain triple loop and gradcheck, GravNetConv's parameters
against PyG's, and the argument errors (raised from shapes, before any device is asked for)."""
import math

import pytest
import torch

from gravnet_reference import RefGravNetConv, aggregate, lowest_slot_argmax, messages

# 7 nodes, k = 4: a full row, rows with -1 at the end / in the middle / at the front, an empty row, a repeated source
NBR7 = torch.tensor([[0, 1, 2, 3],
                     [1, 0, -1, -1],
                     [2, -1, 4, 6],
                     [-1, 3, 5, -1],
                     [-1, -1, -1, -1],
                     [5, 5, 0, 6],
                     [6, 2, 1, 0]], dtype=torch.int32)


def _inputs7(S=3, P=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(7, P, generator=g, dtype=torch.float64)
    s = 0.3 * torch.randn(7, S, generator=g, dtype=torch.float64)
    return h, s


def _loops(h, s_src, s_tgt, nbr):
    Nt, k = nbr.shape
    P = h.shape[1]
    out = [[0.0] * (2 * P) for _ in range(Nt)]
    arg = [[k] * P for _ in range(Nt)]
    bar = [0.0] * Nt
    for i in range(Nt):
        cnt = sum(1 for t in range(k) if int(nbr[i, t]) >= 0)
        for t in range(k):
            j = int(nbr[i, t])
            if j < 0:
                continue
            d = sum((float(s_src[j, c]) - float(s_tgt[i, c])) ** 2 for c in range(s_src.shape[1]))
            w = math.exp(-10.0 * d)
            bar[i] += max(abs(float(v)) for v in h[j])
            for p in range(P):
                m = w * float(h[j, p])
                out[i][p] += m / cnt
                if arg[i][p] == k or m > out[i][P + p]:
                    out[i][P + p] = m
                    arg[i][p] = t
    return torch.tensor(out, dtype=torch.float64), torch.tensor(arg), torch.tensor(bar, dtype=torch.float64)


def test_reference_equals_the_triple_loop():
    h, s = _inputs7()
    out, bar, _msg, _valid, arg = aggregate(h, s, NBR7)
    l_out, l_arg, l_bar = _loops(h, s, s, NBR7)
    torch.testing.assert_close(out, l_out, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(bar, l_bar, rtol=1e-13, atol=0)
    assert torch.equal(arg, l_arg)
    assert torch.equal(out[4], torch.zeros(10, dtype=torch.float64)) and bool((arg[4] == 4).all())


def test_reference_two_sets_equals_the_triple_loop():
    h, s = _inputs7(seed=1)
    s_dst = 0.3 * torch.randn(3, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    nbr = torch.tensor([[6, 0, -1], [-1, -1, -1], [3, 3, 5]], dtype=torch.int32)
    out, bar, *_ = aggregate(h, s, nbr, s_dst)
    l_out, _l_arg, l_bar = _loops(h, s, s_dst, nbr)
    torch.testing.assert_close(out, l_out, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(bar, l_bar, rtol=1e-13, atol=0)


def test_reference_breaks_max_ties_to_the_lowest_slot_and_routes_through_a_given_arg():
    h, s = _inputs7(seed=3)
    msg, valid = messages(h, s, s, NBR7)
    assert bool((lowest_slot_argmax(msg, valid)[5] <= 2).all())      # row 5 lists node 5 in slots 0 and 1: never slot 1
    assert not bool((lowest_slot_argmax(msg, valid)[5] == 1).any())
    hh = h.clone().requires_grad_(True)
    arg = torch.ones(7, 5, dtype=torch.int64)                        # slot 1 everywhere (row 4 is empty: ignored)
    out = aggregate(hh, s, NBR7, arg=arg)[0]
    torch.testing.assert_close(out[5, 5:], msg[5, 1])                # row 5's twin slot carries the same value
    out[:, 5:].sum().backward()
    # row 2's slot 1 is empty: its message is zero and nothing flows; node 0 is slot 1 of row 1 only
    d = (s[0] - s[1]).pow(2).sum()
    torch.testing.assert_close(hh.grad[0], torch.exp(-10 * d).expand(5).clone())


def test_reference_gradcheck():
    h, s = _inputs7(S=2, P=3, seed=4)
    h.requires_grad_(True)
    s.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: aggregate(a, b, NBR7)[0], (h, s), eps=1e-6, atol=1e-6)
    s_dst = (0.3 * torch.randn(7, 2, dtype=torch.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: aggregate(a, b, NBR7, c)[0], (h, s, s_dst), eps=1e-6, atol=1e-6)
    ref = RefGravNetConv(4, 6, 2, 3)
    x = torch.randn(7, 4, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a: ref(a, NBR7), (x,), eps=1e-6, atol=1e-6)


def test_module_parameters_are_pygs():
    import deepmetv2_amd as dm
    conv = dm.GravNetConv(11, 13, 4, 22, 16)
    shapes = {n: tuple(v.shape) for n, v in conv.state_dict().items()}
    assert shapes == {"lin_s.weight": (4, 11), "lin_s.bias": (4,), "lin_h.weight": (22, 11), "lin_h.bias": (22,),
                      "lin_out1.weight": (13, 11), "lin_out2.weight": (13, 44), "lin_out2.bias": (13,)}
    assert repr(conv) == "GravNetConv(11, 13, k=16)"
    assert (conv.in_channels, conv.out_channels, conv.k, conv.num_workers) == (11, 13, 16, None)
    ref = RefGravNetConv(11, 13, 4, 22)
    conv.load_state_dict({n: v.float() for n, v in ref.state_dict().items()})      # strict: the same keys
    before = conv.lin_h.weight.detach().clone()
    conv.reset_parameters()
    assert not torch.equal(before, conv.lin_h.weight)


def test_constructor_limits():
    import deepmetv2_amd as dm
    for bad in (dict(space_dimensions=0), dict(space_dimensions=17), dict(propagate_dimensions=0),
                dict(propagate_dimensions=129), dict(k=0), dict(k=65), dict(k=2.0)):
        kw = dict(space_dimensions=4, propagate_dimensions=22, k=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            dm.GravNetConv(8, 8, **kw)
    dm.GravNetConv(8, 8, 16, 128, 64)       # the limits themselves


def _table(nbr):
    import deepmetv2_amd as dm
    return dm.NeighborTable(nbr, torch.tensor([0, nbr.shape[0]]), dense=False)


def test_aggregate_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    h, s = torch.randn(7, 5), torch.randn(7, 3)
    table = _table(NBR7)
    with pytest.raises(ValueError, match="S=17"):
        dm.gravnet_aggregate(h, torch.randn(7, 17), table)
    with pytest.raises(ValueError, match="P=129"):
        dm.gravnet_aggregate(torch.randn(7, 129), s, table)
    with pytest.raises(ValueError, match="k=65"):
        dm.gravnet_aggregate(h, s, _table(torch.zeros(7, 65, dtype=torch.int32)))
    with pytest.raises(ValueError, match="rows"):
        dm.gravnet_aggregate(torch.randn(6, 5), s, table)
    with pytest.raises(ValueError, match="rows"):
        dm.gravnet_aggregate(h, s, _table(NBR7[:5]))
    with pytest.raises(ValueError, match="s_dst"):
        dm.gravnet_aggregate(h, s, table, s_dst=s)
    with pytest.raises(TypeError):
        dm.gravnet_aggregate(h, s, NBR7)
    # well-formed arguments get as far as the device check: there is no CPU implementation
    with pytest.raises(RuntimeError, match="non-GPU"):
        dm.gravnet_aggregate(h, s, table)


def test_pair_argument_errors_on_cpu_tensors():
    import deepmetv2_amd as dm
    h, s = torch.randn(7, 5), torch.randn(7, 3)
    nbr = torch.tensor([[6, 0, -1], [-1, -1, -1], [3, 3, 5]], dtype=torch.int32)
    ptr = torch.tensor([0, 7]), torch.tensor([0, 3])
    table = dm.BipartiteTable(nbr, ptr[0], ptr[1], 7)
    with pytest.raises(ValueError, match="s_dst"):
        dm.gravnet_aggregate(h, s, table)
    with pytest.raises(ValueError, match="columns"):
        dm.gravnet_aggregate(h, s, table, s_dst=torch.randn(3, 2))
    with pytest.raises(ValueError, match="rows"):
        dm.gravnet_aggregate(h, s, table, s_dst=torch.randn(4, 3))
    with pytest.raises(ValueError, match="candidates"):
        dm.gravnet_aggregate(h[:6], s[:6], table, s_dst=torch.randn(3, 3))
    with pytest.raises(RuntimeError, match="non-GPU"):
        dm.gravnet_aggregate(h, s, table, s_dst=torch.randn(3, 3))
    conv = dm.GravNetConv(4, 4, 2, 3, 2)
    x = torch.randn(7, 4)
    with pytest.raises(ValueError, match="pair"):
        conv(x, (torch.zeros(7, dtype=torch.long), torch.zeros(7, dtype=torch.long)))
    with pytest.raises(ValueError, match="pair"):
        conv((x, x[:3]), torch.zeros(7, dtype=torch.long))
    with pytest.raises(ValueError, match="pair"):
        conv((x, x, x))
    with pytest.raises(ValueError, match="x_l and x_r"):
        conv((x, torch.randn(3, 5)))

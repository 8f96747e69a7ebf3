"""The max / min, sum and clamp lanes of the fused aggregations on rows that hold NaN, +inf and -inf, and the locality of a
non-finite value, forward and backward (csrc/gravnet.hip, multi_aggr.hip, pointnet.hip, interpolate.hip, weighted_sum.hip).
The cases -- one event of 48 nodes, tables of width 8 and 40, source J poisoned in one feature -- and the float64
references: tests/nonfinite_contract.py.

Max / min lanes (GravNet's max half, PointNet's out, PNA min / max): the same bits wherever J stands in the rows that list
it, the reference's value under nan_skipping_max / _min, the reference's winners.  Sum and clamp lanes: the reference's
non-finite pattern.  Finite elements are held to the operators' own bars: GravNet rows 1e-5 bar_i + 1e-6, PointNet 1e-4 of
the largest finite |reference|, PNA min / max exact and pna_reference.bounds for the rest, interpolate (2k + 8) 2^-23 bar,
the weighted sum (n + 2) 2^-24 sum|w x|; every bar is formed from the finite values.  Locality is bit equality with the
clean run.

On the parent of the change that stated the contract: GravNet and PointNet took a NaN that stood in a row's first valid
slot and never let it go (and ignored it anywhere else), PNA reported +-inf with position -1 for a feature whose
candidates were all NaN or all the identity of its min / max, PNA's std was 0 where var was NaN, and interpolate gave a NaN
distance the weight 1e16.
"""
import pytest
import torch

import nonfinite_contract as nc
import pna_reference as pr

pytestmark = pytest.mark.gpu

U23, U24 = 2.0 ** -23, 2.0 ** -24
MAX_OPS = ("gravnet", "pna", "pointnet")
TAKES_LISTS = ("pna", "pointnet", "weighted_sum")


def _graphs(op, nbr, dist, dev):
    """[(form, graph object)]: the table, and the grouped list of the same entries where the operator takes lists."""
    from deepmetv2_amd.graph import NeighborTable, edge_list_from_edge_index
    ptr = torch.tensor([0, nc.AGG_N], dtype=torch.int64, device=dev)
    out = [("table", NeighborTable(nbr.to(dev), ptr, dense=False, dist=dist.to(dev)))]
    if op in TAKES_LISTS:
        i, t = (nbr >= 0).nonzero(as_tuple=True)
        ei = torch.stack([nbr[i, t].long(), i])
        edges = edge_list_from_edge_index(ei.to(dev), nc.AGG_N, "source_to_target")
        assert edges.perm is None and torch.equal(edges.src.cpu().long(), ei[0])
        out.append(("list", edges))
    return out


def _slot_of(win, nbr, form):
    """Winners as table slots (-1 none): a list reports positions among the valid entries, a table i*k + t or t."""
    if form == "table":
        return win
    valid = nbr >= 0
    i, t = valid.nonzero(as_tuple=True)
    slot_of_pos = torch.cat([t, torch.tensor([-1])])
    return slot_of_pos[torch.where(win >= 0, win, torch.full_like(win, t.numel()))]


def _run(op, d, graph, form, nbr, w=None):
    """One forward and backward of `op` on the GPU: dict(lanes={name: fp32 CPU}, win={name: int64 CPU slots, -1 none},
    grads={name: CPU})."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, gravnet
    dev = graph.nbr.device if form == "table" else graph.src.device
    k = nbr.shape[1]
    t = {n: v.to(dev).requires_grad_(n in ("h", "s", "x", "pos")) for n, v in d.items()}
    g = torch.Generator().manual_seed(5)
    if op == "gravnet":
        P = d["h"].shape[1]
        out, arg = gravnet._aggregate(t["h"], t["s"], graph, None)
        out.backward(torch.randn(out.shape, generator=g).to(dev))
        a = arg.cpu().long()
        return dict(lanes={"mean": out[:, :P].detach().cpu(), "max": out[:, P:].detach().cpu()},
                    win={"max": torch.where(a == 255, torch.full_like(a, -1), a)}, grads={"h": t["h"].grad.cpu(), "s": t["s"].grad.cpu()})
    if op == "pna":
        out, _count = dm.multi_aggregate(t["x"], graph, nc.PNA_AGGRS)
        out.backward(torch.randn(out.shape, generator=g).to(dev))
        idx, rowptr = (graph.nbr, None) if form == "table" else (graph.src, graph.rowptr)
        raw, _cnt, (_mean, _var, amin, amax) = _native._multi_aggr_fwd(t["x"].detach(), idx, rowptr, nc.AGG_N, nc.PNA_AGGRS, 1)
        assert torch.equal(raw.view_as(out).isnan(), out.isnan()) and torch.equal(raw.view_as(out).nan_to_num(), out.detach().nan_to_num())
        win = {}
        for name, a in (("min", amin), ("max", amax)):
            a = a.cpu().long()
            win[name] = _slot_of(a, nbr, form) if form == "list" else torch.where(a >= 0, a % k, a)
        return dict(lanes={n: v.float() for n, v in pr.layout(out.detach().cpu(), nc.PNA_AGGRS, 1).items()}, win=win,
                    grads={"x": t["x"].grad.cpu()})
    if op == "pointnet":
        c = nc.POINTNET
        lin1, lin2 = torch.nn.Linear(c["F"] + c["D"], c["H1"]).to(dev), torch.nn.Linear(c["H1"], c["H2"]).to(dev)
        with torch.no_grad():
            for lin, wn, bn in ((lin1, "W1", "b1"), (lin2, "W2", "b2")):
                lin.weight.copy_(t[wn])
                lin.bias.copy_(t[bn])
        out, win = dm.pointnet_aggregate(t["x"], t["pos"], t["pos"], graph, lin1, lin2, c["act"], c["act2"], False,
                                         return_winners=True)
        out.backward(torch.randn(out.shape, generator=g).to(dev))
        return dict(lanes={"out": out.detach().cpu()}, win={"out": _slot_of(win.cpu().long(), nbr, form)},
                    grads={"x": t["x"].grad.cpu(), "pos": t["pos"].grad.cpu()})
    if op == "interpolate":
        out = dm.interpolate_aggregate(t["x"], graph)
        out.backward(torch.randn(out.shape, generator=g).to(dev))
        _raw, wsum = _native.interpolate_fwd(t["x"].detach(), graph.nbr, graph.dist)
        return dict(lanes={"out": out.detach().cpu(), "wsum": wsum.cpu()}, win={}, grads={"x": t["x"].grad.cpu()})
    assert op == "weighted_sum"
    if form == "list":
        w = w.reshape(-1)[(nbr >= 0).flatten()]
    ww = w.to(dev).requires_grad_(True)
    out = dm.weighted_aggregate(t["x"], graph, ww)
    out.backward(torch.randn(out.shape, generator=g).to(dev))
    gw = ww.grad.cpu().reshape(-1)
    if form == "list":        # back to one value per slot, 0 in an empty one
        gw = torch.zeros(nbr.numel()).masked_scatter((nbr >= 0).flatten(), gw)
    return dict(lanes={"out": out.detach().cpu()}, win={}, grads={"x": t["x"].grad.cpu(), "w": gw.view(nc.AGG_N, k)})


def _same_bits(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _within(got, ref, lim, what):
    """same_nonfinite, then |err| <= lim over the elements whose reference is finite; lim must be finite there."""
    nc.same_nonfinite(got, ref, what)
    ok = ref.isfinite()
    lim = lim.expand_as(ref) if torch.is_tensor(lim) else torch.full_like(ref, lim)
    assert bool(lim[ok].isfinite().all()), (what, "bar")
    err = (got.double() - ref).abs()
    assert bool((err[ok] <= lim[ok]).all()), (what, float((err[ok] - lim[ok]).max()))


def _weights(k):
    return torch.randn(nc.AGG_N, k, generator=torch.Generator().manual_seed(3))


def _check_against_reference(op, got, ref, k, what):
    """Every lane of one run against the operator's float64 reference; winners exactly."""
    if op == "gravnet":
        lim = (1e-5 * ref["bar"] + 1e-6).unsqueeze(1)
        _within(got["lanes"]["mean"], ref["mean"], lim, f"{what}: mean")
        _within(got["lanes"]["max"], ref["max"], lim, f"{what}: max")
        assert torch.equal(got["win"]["max"], torch.where(ref["arg"] == 255, torch.full_like(ref["arg"], -1), ref["arg"])), what
    elif op == "pna":
        for a in nc.PNA_AGGRS:
            x, r = got["lanes"][a], ref[a]
            if a in ("min", "max"):
                _within(x, r, 0.0, f"{what}: {a}")
                want = torch.where(ref["arg" + a] >= 0, ref["arg" + a] % k, ref["arg" + a])
                assert torch.equal(got["win"][a], want), (what, "arg" + a)
            elif a == "std":
                big = (ref["var"] > 4e-5) | ~r.isfinite()          # the bound holds clear of the clamp; NaN stays in view
                _within(torch.where(big, x.double(), r), r, ref["bounds"]["std"], f"{what}: std")
                small = ~big
                assert bool((x[small] == 0).all()), (what, "std below the clamp")
            else:
                _within(x, r, ref["bounds"][a], f"{what}: {a}")
    elif op == "pointnet":
        _within(got["lanes"]["out"], ref["out"], 1e-4 * ref["scale"], f"{what}: out")
        assert torch.equal(got["win"]["out"], ref["win"]), (what, "win")
    elif op == "interpolate":
        _within(got["lanes"]["out"], ref["out"], (2 * k + 8) * U23 * ref["bar"] + 1e-30, f"{what}: out")
        nc.same_nonfinite(got["lanes"]["wsum"], ref["wsum"], f"{what}: wsum")
        ok = ref["wsum"].isfinite()
        assert bool(((got["lanes"]["wsum"].double() - ref["wsum"]).abs()[ok] <= (k + 2) * U23 * ref["wsum"][ok]).all()), (what, "wsum")
    else:
        _within(got["lanes"]["out"], ref["out"], ref["bound"], f"{what}: out")


# ---- order independence of the max / min lanes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", list(nc.POISONS))
@pytest.mark.parametrize("k", nc.WIDTHS)
@pytest.mark.parametrize("op", MAX_OPS)
def test_max_and_min_do_not_depend_on_where_the_value_stands(dev, op, k, poison):
    nbr0, dist0 = nc.agg_table(k)
    d = nc.agg_inputs(op, nc.POISONS[poison])
    lanes = {"gravnet": ("max",), "pna": ("min", "max"), "pointnet": ("out",)}[op]
    first = None
    for slot in nc.PLACEMENTS[k]:
        nbr, dist, shift = nc.rotate(nbr0, dist0, slot)
        assert all(int(nbr[i, slot]) == nc.J for i in nc.LISTING)
        ref = nc.agg_reference(op, d, nbr, dist)
        for form, graph in _graphs(op, nbr, dist, dev):
            what = f"{op}, k={k}, {poison}, J in slot {slot}, {form}"
            got = _run(op, d, graph, form, nbr)
            _check_against_reference(op, got, ref, k, what)
            if first is None:
                first = (got, shift)
            for a in lanes:
                assert _same_bits(got["lanes"][a], first[0]["lanes"][a]), (what, a, "bits")
                # the winners, mapped through the rotation
                was, rel = first[0]["win"][a], (shift - first[1]).view(-1, 1)
                assert torch.equal(got["win"][a], torch.where(was >= 0, (was + rel) % k, was)), (what, a, "winners")
            # the row whose candidates are all J
            row = {a: got["lanes"][a][nc.ALL_J] for a in lanes}
            wins = {a: got["win"][a][nc.ALL_J] for a in lanes}
            f = nc.FEATURE
            if op != "pointnet":
                for a in lanes:
                    if poison == "nan":
                        assert bool(row[a][f].isnan()) and int(wins[a][f]) == -1, (what, a, "all NaN")
                    else:
                        assert float(row[a][f]) == nc.POISONS[poison] and int(wins[a][f]) == 0, (what, a, "all " + poison)
                    rest = torch.arange(row[a].numel()) != f
                    assert bool(row[a][rest].isfinite().all()) and bool((wins[a][rest] == 0).all()), (what, a)
            elif poison == "nan":        # ELU carries the NaN into every message of J
                assert bool(row["out"].isnan().all()) and bool((wins["out"] == -1).all()), (what, "all NaN")
            # in the rows that list J among numbers no max / min lane is NaN
            listing = torch.tensor(nc.LISTING)
            for a in lanes:
                assert not bool(got["lanes"][a][listing].isnan().any()), (what, a, "a NaN won or blocked")


# ---- visibility in the sum and clamp lanes, locality everywhere ----------------------------------------------------------------
@pytest.mark.parametrize("poison", list(nc.POISONS))
@pytest.mark.parametrize("k", nc.WIDTHS)
@pytest.mark.parametrize("op", nc.AGG_OPS)
def test_a_poisoned_source_shows_where_it_is_listed_and_nowhere_else(dev, op, k, poison):
    nbr, dist = nc.agg_table(k)
    lists, shares, apart = nc.agg_masks(nbr)
    w = _weights(k)
    clean_d, bad_d = nc.agg_inputs(op), nc.agg_inputs(op, nc.POISONS[poison])
    ref = nc.agg_reference(op, bad_d, nbr, dist, w)
    f = nc.FEATURE
    for form, graph in _graphs(op, nbr, dist, dev):
        what = f"{op}, k={k}, {poison}, {form}"
        clean, bad = _run(op, clean_d, graph, form, nbr, w), _run(op, bad_d, graph, form, nbr, w)
        assert all(bool(v.isfinite().all()) for v in list(clean["lanes"].values()) + list(clean["grads"].values())), what
        _check_against_reference(op, bad, ref, k, what)
        # visibility: the sum and clamp lanes of the poisoned feature in the rows that list J
        sums = {"gravnet": ("mean",), "pna": ("sum", "mean", "var", "std"), "pointnet": (), "interpolate": ("out",),
                "weighted_sum": ("out",)}[op]
        for a in sums:
            col = bad["lanes"][a][lists][:, f]
            assert not bool(col.isfinite().any()), (what, a, "hidden")
            if poison == "nan":
                assert bool(col.isnan().all()), (what, a)
        # locality, forward: every other row, and (per-feature operators) every other feature, has the clean run's bits
        for a, v in bad["lanes"].items():
            assert torch.equal(v[~lists], clean["lanes"][a][~lists]), (what, a, "another row moved")
            if op != "pointnet" and v.dim() == 2:
                rest = torch.arange(v.shape[1]) != f
                assert torch.equal(v[:, rest], clean["lanes"][a][:, rest]), (what, a, "another feature moved")
        for a, v in bad["win"].items():
            assert torch.equal(v[~lists], clean["win"][a][~lists]), (what, a, "another row's winner moved")
        # locality, backward: a source or target that shares no row with J
        for a, v in bad["grads"].items():
            assert torch.equal(v[apart], clean["grads"][a][apart]), (what, "g_" + a, "a gradient row apart from J moved")
        if op == "weighted_sum":
            assert torch.equal(bad["grads"]["w"][~lists], clean["grads"]["w"][~lists]), what


# ---- interpolate: the distances are an input ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", nc.WIDTHS)
def test_a_nan_distance_takes_its_row_and_an_empty_slot_takes_nothing(dev, k):
    nbr, dist = nc.agg_table(k)
    d = nc.agg_inputs("interpolate")
    (_form, table), = _graphs("interpolate", nbr, dist, dev)
    clean = _run("interpolate", d, table, "table", nbr)
    # NaN (and +-inf) in the distance of every empty slot: no bit moves
    for val in nc.POISONS.values():
        dist_e = dist.clone()
        dist_e[nbr < 0] = val
        assert int((nbr < 0).sum()) > k
        (_f, t2), = _graphs("interpolate", nbr, dist_e, dev)
        got = _run("interpolate", d, t2, "table", nbr)
        for a in ("out", "wsum"):
            assert torch.equal(got["lanes"][a], clean["lanes"][a]), (k, a, "an empty slot's distance was read")
        assert torch.equal(got["grads"]["x"], clean["grads"]["x"]), k
    # NaN in one valid slot, first, in the middle of a chunk and last: the whole row is NaN, forward and in g_x of its sources
    row = 30
    assert bool((nbr[row] >= 0).all()) and not bool((nbr[row] == nc.J).any())
    for slot in (0, k // 2, k - 1):
        dist_n = dist.clone()
        dist_n[row, slot] = nc.NAN
        (_f, t3), = _graphs("interpolate", nbr, dist_n, dev)
        got = _run("interpolate", d, t3, "table", nbr)
        ref = nc.agg_reference("interpolate", d, nbr, dist_n)
        what = f"interpolate, k={k}, NaN distance in slot {slot}"
        _check_against_reference("interpolate", got, ref, k, what)
        assert bool(got["lanes"]["out"][row].isnan().all()) and bool(got["lanes"]["wsum"][row].isnan()), what
        others = torch.arange(nc.AGG_N) != row
        for a in ("out", "wsum"):
            assert torch.equal(got["lanes"][a][others], clean["lanes"][a][others]), (what, a)
        in_row = torch.zeros(nc.AGG_N, dtype=torch.bool)
        in_row[nbr[row].long()] = True
        assert bool(got["grads"]["x"][in_row].isnan().all()), what
        assert torch.equal(got["grads"]["x"][~in_row], clean["grads"]["x"][~in_row]), what

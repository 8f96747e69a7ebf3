"""The non-finite contract's cases without a GPU: every case of tests/nonfinite_contract.py builds, its float64 reference has
exactly the stated pattern, every bar is finite, and an fp32 emulation of the chunked running softmax shows which
recurrence meets the contract -- the parent's does not (a first chunk of dead entries poisons the row), a restart at
m == -inf does not (it erases a NaN score), the stated one does.
"""
import inspect
import re

import numpy as np
import pytest
import torch

import nonfinite_contract as nc

# S6 (D x (c-1), L, D x (c+2)) is not among them: its live entry is the last of the first chunk, so m is finite from there
FINITE_FAILS_ON_PARENT = {"S1", "S2", "S3", "S11 empty, dead, live", "S11 dead, empty, live", "S12 dead row, live self",
                          "S12 written self among the dead"}


def _logical_row(row, self_loops, dead_self=False):
    """The row as the kernels walk it under self_loops: a written self loop is an empty slot, the self entry follows."""
    if not self_loops:
        return row
    return [("E" if m == "S" else m, n) for m, n in row] + [("D" if dead_self else "L", 1)]


@pytest.mark.parametrize("c", list(nc.CHUNKS))
def test_the_running_softmax_in_three_forms(c):
    failing = {"parent": set(), "restart": set(), "contract": set()}
    for at, (name, (row, which, loops)) in enumerate(nc.softmax_rows(c).items()):
        s, ok, v = nc.row_scores(_logical_row(row, loops, name.endswith("dead self")), seed=at)
        r_out, r_lse, r_alpha = nc.softmax_f64(s, ok, v)
        assert np.isfinite([r_out, r_lse]).all() == (which == "finite"), name
        assert np.isfinite(r_alpha).all() == (which == "finite"), name
        if which == "nan":
            assert np.isnan(r_out) and np.isnan(r_lse) and np.isnan(r_alpha[ok]).all(), name
        for form in failing:
            out, lse, alpha = nc.chunked_softmax(s, ok, v, c, form)
            got, ref = np.concatenate([[out, lse], alpha]).astype(np.float64), np.concatenate([[r_out, r_lse], r_alpha])
            if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.allclose(got, ref, rtol=1e-5, atol=1e-6, equal_nan=True)):
                failing[form].add(name)
    # at c = 32 the table of k = 64 has no room for (E x c, D x c, L): its dead run ends in the chunk that holds the live entry
    fails = FINITE_FAILS_ON_PARENT - ({"S11 empty, dead, live"} if c == 32 else set())
    assert failing["parent"] == fails, failing["parent"]
    assert failing["restart"] == {"S8"}, failing["restart"]
    assert failing["contract"] == set(), failing["contract"]


def test_a_finite_row_has_the_parents_bits_in_the_contract_form():
    rng = np.random.default_rng(3)
    for n in (1, 15, 16, 17, 33, 70):
        s, v = rng.standard_normal(n).astype(np.float32) * 8, rng.standard_normal(n).astype(np.float32)
        ok = rng.random(n) > 0.2
        ok[0] = True
        for c in nc.CHUNKS:
            a, b = nc.chunked_softmax(s, ok, v, c, "parent"), nc.chunked_softmax(s, ok, v, c, "contract")
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (n, c)


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("which", ["finite", "nan"])
@pytest.mark.parametrize("c", list(nc.CHUNKS))
def test_softmax_graphs_build_and_their_references_have_the_stated_pattern(c, which, loops):
    graph = nc.softmax_graph(c, which, loops)
    tgt, src = nc.list_form(graph)
    nbr, fits = nc.table_form(graph)
    assert len(graph["rows"]) == nc.NODES and nbr.shape == (nc.NODES, nc.TABLE_K[c]) and fits
    expected = {n: w for n, (_r, w, s) in nc.softmax_rows(c).items() if s == loops}
    assert set(graph["target"]) == {n for n, w in expected.items() if w == which}
    case_rows = torch.tensor(sorted(graph["target"].values()))
    for op in nc.OPS if not loops else nc.OPS[1:]:
        ins = [t.double().requires_grad_(True) for t in nc.softmax_inputs(op, c, self_loops=loops)]
        ref = nc.softmax_reference(op, ins, tgt, src, loops)
        assert bool(ref["bar"].isfinite().all()) and bool((ref["bar"][case_rows] > 0).all() or which == "nan"), op
        # v2 and attention carry the special value in channel 0 of an operand of the output or of a gradient; the
        # channels beyond it, and all of v1, have exactly the stated pattern
        out = ref["out"].detach() if op != "gat_v2" else ref["out"].detach()[:, :, 1:]
        rows_nan = out.isnan().flatten(1).any(1)
        want = torch.zeros(nc.NODES, dtype=torch.bool)
        if which == "nan":
            want[case_rows] = True
        assert torch.equal(rows_nan, want), (op, rows_nan.nonzero().flatten().tolist())
        assert torch.equal(ref["lse"].isnan().any(1), want) and bool(out[want].isnan().all()), op
        in_case = torch.isin(ref["tgt"], case_rows)
        assert bool(ref["alpha"][in_case].isnan().all()) if which == "nan" else bool(ref["alpha"].isfinite().all()), op
        assert bool(ref["alpha"][~in_case].isfinite().all()), op
        if op == "gat_v1" and which == "finite":
            g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
            ref["out"].backward(g)
            assert all(bool(t.grad.isfinite().all()) for t in ins)
            dead = torch.tensor(nc.DEAD)
            assert bool((ins[1].grad[dead] == 0).all())         # a dead source's score moves nothing


def test_s1_is_one_live_entry_after_a_dead_chunk():
    for c in nc.CHUNKS:
        graph = nc.softmax_graph(c, "finite")
        tgt, src = nc.list_form(graph)
        ins = [t.double() for t in nc.softmax_inputs("gat_v1", c)]
        ref = nc.softmax_reference("gat_v1", ins, tgt, src)
        t = graph["target"]["S1"]
        row = graph["rows"][t]
        assert len(row) == c + 1 and all(j in nc.DEAD for j in row[:c]) and row[c] in nc.LIVE
        assert torch.equal(ref["out"][t], ins[0][row[c]])
        assert ref["alpha"][ref["tgt"] == t].T.tolist() == [[0.0] * c + [1.0]] * nc.CHUNKS[c][0]


def test_nan_skipping_max_and_min():
    nan, inf = nc.NAN, nc.INF
    v = torch.tensor([[nan, 2.0, 5.0, 5.0], [nan, nan, nan, 7.0], [-inf, -inf, nan, -inf], [1.0, inf, nan, inf],
                      [3.0, 1.0, 2.0, 0.0]])
    ok = torch.ones_like(v, dtype=torch.bool)
    ok[1, 3] = False
    ok[4] = False
    val, pos = nc.nan_skipping_max(v, ok)
    assert pos.tolist() == [2, -1, 0, 1, -1] and val[[0, 2, 3, 4]].tolist() == [5.0, -inf, inf, 0.0] and bool(val[1].isnan())
    val, pos = nc.nan_skipping_min(v, ok)
    assert pos.tolist() == [1, -1, 0, 0, -1] and val[[0, 2, 3, 4]].tolist() == [2.0, -inf, 1.0, 0.0] and bool(val[1].isnan())


def test_same_nonfinite_tells_the_patterns_apart():
    ref = torch.tensor([1.0, nc.NAN, nc.INF, -nc.INF])
    nc.same_nonfinite(torch.tensor([2.0, nc.NAN, nc.INF, -nc.INF]), ref)
    for bad in ([nc.NAN, nc.NAN, nc.INF, -nc.INF], [1.0, 0.0, nc.INF, -nc.INF], [1.0, nc.NAN, -nc.INF, -nc.INF],
                [1.0, nc.NAN, nc.INF, 0.0], [nc.INF, nc.NAN, nc.INF, -nc.INF]):
        with pytest.raises(AssertionError):
            nc.same_nonfinite(torch.tensor(bad), ref)


def test_the_table_names_every_aggregation_entry():
    """Every forward entry of _native.py that walks a neighbour row with a running state is in ENTRIES, held or excused."""
    from deepmetv2_amd import _native
    named = {n.lstrip("_") for n, f in inspect.getmembers(_native, inspect.isfunction)
             if re.fullmatch(r"_?(attention|gat|gravnet|multi_aggr|pointnet|interpolate|weighted_sum)_fwd", n)}
    assert named == set(nc.ENTRIES), named ^ set(nc.ENTRIES)
    assert all(isinstance(why, str) and why for why in nc.ENTRIES.values())


# ---- the max / min, clamp and locality cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", nc.WIDTHS)
def test_aggregate_tables_and_the_rotation(k):
    nbr, dist = nc.agg_table(k)
    lists, shares, apart = nc.agg_masks(nbr)
    assert lists.nonzero().flatten().tolist() == sorted(nc.LISTING + (nc.ALL_J,)) and bool((nbr[nc.ALL_J] == nc.J).all())
    assert not bool(shares[40:].any()) and bool((nbr[-1] < 0).all()) and bool((nbr[1, k - 3:] < 0).all())
    for i in range(nc.AGG_N):          # distinct sources inside a row (but the all-J row): no exact tie of two entries
        ids = nbr[i][nbr[i] >= 0].tolist()
        assert i == nc.ALL_J or len(set(ids)) == len(ids)
    assert max(nc.PLACEMENTS[k]) == k - 1 and all(c - 1 in nc.PLACEMENTS[k] and c in nc.PLACEMENTS[k] for c in (16, 32) if c < k)
    for slot in nc.PLACEMENTS[k]:
        rot, rdist, shift = nc.rotate(nbr, dist, slot)
        assert all(int(rot[i, slot]) == nc.J for i in nc.LISTING)
        for i in range(nc.AGG_N):      # every row keeps its entries, each with its own distance
            assert sorted(zip(rot[i].tolist(), rdist[i].tolist())) == sorted(zip(nbr[i].tolist(), dist[i].tolist()))
            if i not in nc.LISTING:
                assert torch.equal(rot[i], nbr[i]) and int(shift[i]) == 0
            else:
                assert torch.equal(rot[i].roll(-int(shift[i])), nbr[i])


@pytest.mark.parametrize("poison", [None] + list(nc.POISONS))
@pytest.mark.parametrize("k", nc.WIDTHS)
def test_aggregate_references_have_the_stated_pattern_and_finite_bars(k, poison):
    nbr, dist = nc.agg_table(k)
    lists, _shares, _apart = nc.agg_masks(nbr)
    val = None if poison is None else nc.POISONS[poison]
    f = nc.FEATURE
    other = torch.arange(nc.FEATURES) != f
    w = torch.randn(nc.AGG_N, k, generator=torch.Generator().manual_seed(3))
    refs = {op: nc.agg_reference(op, nc.agg_inputs(op, val), nbr, dist, w) for op in nc.AGG_OPS}
    # the bars are finite wherever they are applied
    g = refs["gravnet"]
    assert bool(g["bar"].isfinite().all())
    p = refs["pna"]
    for a in ("sum", "mean", "var", "std"):
        assert bool(p["bounds"][a][p[a].isfinite()].isfinite().all()), a
    v = p["var"][p["var"].isfinite() & (p["count"] > 0).view(-1, 1)]
    assert bool(((v == 0) | (v < 2.5e-6) | (v > 4e-5)).all())        # no finite variance near the clamp of std
    assert refs["pointnet"]["scale"] > 0 and refs["pointnet"]["scale"] < float("inf")
    assert bool(refs["interpolate"]["bar"].isfinite().all())
    ws = refs["weighted_sum"]
    assert bool(ws["bound"][ws["out"].isfinite()].isfinite().all())
    # the patterns: only the poisoned feature of the rows that list J is touched; max / min skip a NaN
    for lane in (g["mean"], g["max"], p["sum"], p["mean"], p["min"], p["max"], p["var"], p["std"], refs["interpolate"]["out"],
                 ws["out"]):
        bad = ~lane.isfinite()
        assert not bool(bad[~lists].any()) and not bool(bad[:, torch.arange(lane.shape[1]) != f].any())
    if poison is None:
        return
    for lane in (g["mean"], p["sum"], p["mean"], p["var"], p["std"], refs["interpolate"]["out"], ws["out"]):
        assert not bool(lane[lists][:, f].isfinite().any())
    listing = torch.tensor(nc.LISTING)
    for lane, arg, none in ((g["max"], g["arg"], 255), (p["min"], p["argmin"], -1), (p["max"], p["argmax"], -1)):
        assert not bool(lane[listing].isnan().any()) and bool((arg[listing] != none).all())
        if poison == "nan":
            assert bool(lane[nc.ALL_J, f].isnan()) and int(arg[nc.ALL_J, f]) == none
        else:
            assert float(lane[nc.ALL_J, f]) == val and int(arg[nc.ALL_J, f]) in (0, nc.ALL_J * k)
    pn = refs["pointnet"]
    assert not bool(pn["out"][listing].isnan().any())
    if poison == "nan":
        assert bool(pn["out"][nc.ALL_J].isnan().all()) and bool((pn["win"][nc.ALL_J] == -1).all())


@pytest.mark.parametrize("k", nc.WIDTHS)
def test_no_winner_of_a_max_lane_depends_on_fp32_rounding(k):
    """What lets the GPU tests hold the winners to the reference's exactly (see AGG_SEED)."""
    import gravnet_reference as gvr
    nbr, dist = nc.agg_table(k)
    rows = torch.ones(nc.AGG_N, dtype=torch.bool)
    rows[nc.ALL_J] = False          # k copies of one entry: an exact tie on every machine, the lowest slot wins (R4)
    for val in [None] + list(nc.POISONS.values()):
        d = nc.agg_inputs("gravnet", val)
        msg, valid = gvr.messages(d["h"].double(), d["s"].double(), d["s"].double(), nbr)
        m = torch.where(valid.unsqueeze(-1) & ~msg.isnan(), msg, torch.full_like(msg, -nc.INF))
        top = m.topk(2, dim=1).values
        rel = ((top[:, 0] - top[:, 1]) / torch.maximum(top[:, 0].abs(), top[:, 1].abs()))[rows & valid.any(1)]
        assert bool((rel[rel.isfinite()] > 1e-3).all()), float(rel[rel.isfinite()].min())
        bare = nbr.clone()
        bare[nc.ALL_J] = -1
        assert nc.agg_reference("pointnet", nc.agg_inputs("pointnet", val), bare)["fragile"] == 0

"""The softmax lanes of attention_aggregate, gat_v1_aggregate and gat_aggregate on rows that hold scores of -inf, +inf and
NaN, wherever in the row they stand and however the row falls into chunks (csrc/row_softmax.h, softmax_row_fwd), against
the operators' float64 references over the same entries.  The cases, their graphs and inputs: tests/nonfinite_contract.py.

Checked: out, alpha, lse (through _native) and the three gradients of each operator.  Non-finite elements: the reference's
NaN mask and infinities (same_nonfinite).  Finite elements: the operators' own bars -- output rows
|err| <= 1e-5 bar_i + 1e-6 with bar_i the largest finite |v_j| over the entries that carry weight, alpha rtol 1e-4 atol
1e-6, gradients rtol 1e-4 atol 1e-4 max|finite ref|.  lse is held to |err| <= 1e-5 (|lse| + 1): a score is a sum of at
most 40 products of order 1 / sqrt(C) formed in fp32 (C u times the sum of their sizes, below 3e-6 here), expf and logf
add a few ulp.

On the parent of the change that stated the contract the finite cases S1, S2, S3, S11 and S12 failed: a first chunk of
nothing but dead entries left l = acc = NaN, which the next chunk's rescaling by 0 kept.
"""
import pytest
import torch

import attention_reference as ar
import gat_reference as gr
import nonfinite_contract as nc

pytestmark = pytest.mark.gpu


def _forms(graph, dev, bipartite=False):
    """(name, graph object, tgt, src, pos or None, the cases present) of the list, the table and (attention) the
    bipartite table of one case graph.  The list keeps the written order: that is asserted from its src."""
    from deepmetv2_amd.graph import BipartiteTable, NeighborTable, edge_list_from_edge_index
    tgt, src = nc.list_form(graph)
    edges = edge_list_from_edge_index(torch.stack([src, tgt]).to(dev), nc.NODES, "source_to_target")
    assert edges.perm is None and torch.equal(edges.src.cpu().long(), src) and torch.equal(edges.tgt.cpu().long(), tgt)
    forms = [("list", edges, tgt, src, None, list(graph["target"]))]
    nbr, fits = nc.table_form(graph)
    t_tgt, t_src, pos = ar.table_entries(nbr, nc.NODES)
    ptr = torch.tensor([0, nc.NODES], dtype=torch.int32, device=dev)
    forms.append(("table", NeighborTable(nbr.to(dev), ptr, dense=False), t_tgt, t_src, pos, fits))
    if bipartite:
        forms.append(("bipartite table", BipartiteTable(nbr.to(dev), ptr, ptr, nc.NODES), t_tgt, t_src, pos, fits))
    return forms


def _gpu(op, ins, graph, self_loops=False):
    """(out, alpha [positions, H], lse, gradients, g) of `op` on the GPU: the public aggregate and its backward, lse from
    the native forward, whose out and alpha must be the aggregate's bits."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    from deepmetv2_amd._softmax_conv import graph_args
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    idx, rowptr, _tgt = graph_args(graph)
    if op == "attention":
        out, alpha = dm.attention_aggregate(*leaves, graph, return_alpha=True)
        n_out, lse, n_alpha = _native.attention_fwd(*ins, idx, rowptr, True)
    else:
        fn, mode = (dm.gat_v1_aggregate, _native.GAT_V1) if op == "gat_v1" else (dm.gat_aggregate, _native.GAT_V2)
        out, alpha = fn(*leaves, graph, negative_slope=nc.SLOPE, self_loops=self_loops, return_alpha=True)
        n_out, lse, n_alpha = _native._gat_fwd(mode, *ins, idx, rowptr, nc.SLOPE, self_loops, True)
    alpha = alpha.reshape(-1, alpha.shape[-1])
    for a, b in ((out.detach(), n_out), (alpha, n_alpha)):
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    out.backward(g)
    return out.detach().cpu(), alpha.cpu(), lse.cpu(), [t.grad.cpu() for t in leaves], g.cpu()


def _check(op, ins, graph, tgt, src, pos, self_loops=False, what=""):
    """Everything of `op` over one graph form against the float64 reference; returns what the GPU and the reference gave."""
    out, alpha, lse, grads, g = _gpu(op, ins, graph, self_loops)
    ins64 = [t.detach().cpu().double().requires_grad_(True) for t in ins]
    ref = nc.softmax_reference(op, ins64, tgt, src, self_loops)
    assert out.dtype == torch.float32
    nc.check_output(out, ref["out"], ref["bar"], f"{what}: out")
    # alpha of the written entries: the reference's, 0 in an empty slot and in a written self loop that was skipped
    a = alpha.double()
    if pos is not None:
        assert bool((a[torch.ones(a.shape[0], dtype=torch.bool).index_fill(0, pos, False)] == 0).all()), what
        a = a[pos]
    kept = (tgt != src) if self_loops else torch.ones_like(tgt, dtype=torch.bool)
    r_written = torch.zeros_like(a)
    r_written[kept] = ref["alpha"].detach()[:int(kept.sum())]
    nc.same_nonfinite(a, r_written, f"{what}: alpha")
    torch.testing.assert_close(*nc.finite_pair(a, r_written), rtol=1e-4, atol=1e-6, msg=lambda m: f"{what}: alpha: {m}")
    nc.same_nonfinite(lse, ref["lse"], f"{what}: lse")
    l_got, l_ref = nc.finite_pair(lse, ref["lse"])
    assert bool(((l_got - l_ref).abs() <= 1e-5 * (l_ref.abs() + 1)).all()), (what, "lse", float((l_got - l_ref).abs().max()))
    ref["out"].backward(g.double())
    for n, (x, leaf) in enumerate(zip(grads, ins64)):
        nc.check_grad(x, leaf.grad, f"{what}: gradient {n}")
    return dict(out=out, alpha=a, lse=lse, grads=grads, ref=ref, ref_alpha=r_written, ref_grads=[t.grad for t in ins64])


def _entries_of(tgt, t):
    return (tgt == t).nonzero().flatten()


@pytest.mark.parametrize("which", ["finite", "nan"])
@pytest.mark.parametrize("c", list(nc.CHUNKS))
@pytest.mark.parametrize("op", nc.OPS)
def test_placement_cases(dev, op, c, which):
    """S1 to S11 in the list, the table and (attention) a bipartite table."""
    graph = nc.softmax_graph(c, which)
    ins = [t.to(dev) for t in nc.softmax_inputs(op, c)]
    values = (ins[2] if op == "attention" else ins[0]).cpu()
    for form, gobj, tgt, src, pos, present in _forms(graph, dev, bipartite=op == "attention"):
        what = f"{op}, c={c}, {which}, {form}"
        got = _check(op, ins, gobj, tgt, src, pos, what=what)
        assert present, what
        for case in present:
            t = graph["target"][case]
            e = _entries_of(tgt, t)
            rest = slice(1, None) if op == "gat_v2" else slice(None)         # v2: channel 0 of out is 0 * -inf
            if which == "nan":
                assert bool(got["out"][t].isnan().all()) and bool(got["lse"][t].isnan().all()), (what, case)
                assert e.numel() and bool(got["alpha"][e].isnan().all()), (what, case)
            else:
                assert bool(got["out"][t][:, rest].isfinite().all()) and bool(got["lse"][t].isfinite().all()), (what, case)
                assert bool(got["alpha"][e].isfinite().all()), (what, case)
                dead = torch.isin(src[e], torch.tensor(nc.DEAD))
                assert bool((got["alpha"][e][dead] == 0).all()), (what, case)         # -inf beside a finite score: exactly 0
            if case == "S1":
                j = graph["rows"][t][-1]
                assert torch.equal(got["out"][t][:, rest], values[j][:, rest]), (what, "S1: out is v_j")
                assert got["alpha"][e].T.tolist() == [[0.0] * c + [1.0]] * nc.CHUNKS[c][0], (what, "S1: alpha")
        if which == "finite" and op == "gat_v1":
            assert all(bool(x.isfinite().all()) for x in got["grads"]), what
            assert bool((got["grads"][1][nc.DEAD] == 0).all()), what


@pytest.mark.parametrize("which", ["finite", "nan"])
@pytest.mark.parametrize("c", list(nc.CHUNKS))
@pytest.mark.parametrize("op", nc.OPS[1:])
def test_self_loops_after_a_dead_chunk(dev, op, c, which):
    """S12: c dead written entries and the implicit self entry alone in the second chunk."""
    graph = nc.softmax_graph(c, which, self_loops=True)
    ins = [t.to(dev) for t in nc.softmax_inputs(op, c, self_loops=True)]
    xl = ins[0].cpu()
    for form, gobj, tgt, src, pos, present in _forms(graph, dev):
        what = f"{op}, c={c}, {which}, self loops, {form}"
        got = _check(op, ins, gobj, tgt, src, pos, self_loops=True, what=what)
        assert set(present) == set(graph["target"]), what
        self_alpha = got["ref"]["alpha"].detach()[int((tgt != src).sum()):]
        for case, t in graph["target"].items():
            e = _entries_of(tgt, t)
            if which == "nan":
                assert bool(got["out"][t].isnan().all()) and bool(got["lse"][t].isnan().all()), (what, case)
                assert bool(got["alpha"][e[src[e] != t]].isnan().all()), (what, case)
                continue
            rest = slice(1, None) if op == "gat_v2" else slice(None)
            assert torch.equal(got["out"][t][:, rest], xl[t][:, rest]), (what, case, "out is xl[i]")
            assert bool((got["alpha"][e] == 0).all()) and bool((self_alpha[t] == 1).all()), (what, case)
            if "written self" in case:
                assert int((src[e] == t).sum()) == 1, (what, case)
            score = nc.softmax_scores(op, [x.cpu().double() for x in ins], torch.tensor([t]), torch.tensor([t]))[0]
            assert bool(((got["lse"][t].double() - score).abs() <= 1e-5 * (score.abs() + 1)).all()), (what, case, "lse")
        if which == "finite" and op == "gat_v1":
            assert all(bool(x.isfinite().all()) for x in got["grads"]), what


@pytest.mark.parametrize("c", list(nc.CHUNKS))
@pytest.mark.parametrize("op", nc.OPS)
def test_the_same_rows_with_every_source_live(dev, op, c):
    """The control: no special value anywhere.  Everything is finite and meets the bars; the list and the table give the
    same bits in the rows both hold (the same entries in the same order)."""
    graph = nc.softmax_graph(c, "finite")
    ins = [t.to(dev) for t in nc.softmax_inputs(op, c, all_live=True)]
    outs = {}
    for form, gobj, tgt, src, pos, present in _forms(graph, dev):
        got = _check(op, ins, gobj, tgt, src, pos, what=f"{op}, c={c}, all live, {form}")
        assert all(bool(x.isfinite().all()) for x in [got["out"], got["alpha"], got["lse"]] + got["grads"])
        outs[form] = got
    nbr, _fits = nc.table_form(graph)
    full = (nbr >= 0).sum(1)
    both = (full > 0) & ((nbr[:, :1] >= 0) & (nbr >= 0).long().diff(dim=1).le(0).all(1, keepdim=True)).squeeze(1)
    assert 0 < int(both.sum()) < nc.NODES         # a row with empty slots before its entries falls into other chunks
    assert torch.equal(outs["list"]["out"][both], outs["table"]["out"][both])
    assert torch.equal(outs["list"]["lse"][both], outs["table"]["lse"][both])

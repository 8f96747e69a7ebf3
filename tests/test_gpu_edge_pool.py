"""Edge pooling on the GPU: the matching kernel against the sequential rule of tests/edge_pool_reference.py (equality, both
state forms), its bit rules, its deferred checks, and the EdgePooling layer -- its partition against the rule run on the
scores it returned itself, its values and gradients against the float64 restatement on that same partition.

Tolerances of the layer, per tensor: 4 times the largest error of the same formulas composed from fp32 torch operators on
the CPU against float64, plus 1e-6 of the tensor's largest magnitude (the convention of tests/test_gpu_weighted_sum.py);
every check prints its error / tolerance ratio before it asserts."""
import warnings

import numpy as np
import pytest
import torch

import edge_pool_reference as er
from poisoned_alloc import run_both, to_bytes

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in er.all_cases()}
FORMS = ("lds", "workspace")


@pytest.fixture(autouse=True)
def _drain():
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()
    yield
    dm.raise_deferred_errors()


@pytest.fixture(scope="module")
def rule():
    """The sequential rule and the emulated round counts of every case, computed once."""
    out = {}
    for name, c in CASES.items():
        args = (c.edge_index[0], c.edge_index[1], c.score, np.arange(c.edge_index.shape[1]), er.ptr_of(c.sizes), sum(c.sizes))
        out[name] = er.sequential_match(*args) + (er.round_match(*args)[3],)
    return out


def _form(monkeypatch, form):
    if form == "workspace":
        monkeypatch.setenv("DMET_EDGE_MATCH_STATE", "workspace")
    else:
        monkeypatch.delenv("DMET_EDGE_MATCH_STATE", raising=False)


def _native_args(case, dev):
    """The grouped operands of _native._edge_match for a case whose targets are in range."""
    N = sum(case.sizes)
    rowptr, src, tgt, perm = er.group_by_target(case.edge_index, N)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return t(rowptr), t(src), t(tgt), t(perm), t(case.score[perm]), t(er.ptr_of(case.sizes))


def _batch(dev, sizes):
    import deepmetv2_amd as dm
    sz = torch.tensor(sizes, dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sz.cumsum(0)])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sz).to(dev)
    dm.register_batch(batch, ptr.to(dev), len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    return batch


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((to_bytes(a) == to_bytes(b)).all())


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(CASES))
def test_matching_equals_the_sequential_rule(dev, monkeypatch, rule, name, form):
    from deepmetv2_amd import _native
    _form(monkeypatch, form)
    case = CASES[name]
    cluster, partner, edge, rounds, flags = _native._edge_match(*_native_args(case, dev), want_rounds=True)
    want = rule[name]
    assert cluster.dtype == edge.dtype == torch.int64 and partner.dtype == rounds.dtype == torch.int32
    assert torch.equal(cluster.cpu(), torch.from_numpy(want[0]))
    assert torch.equal(partner.cpu().long(), torch.from_numpy(want[1]))
    assert torch.equal(edge.cpu(), torch.from_numpy(want[2]))
    assert rounds.cpu().tolist() == want[3].tolist()
    assert flags.cpu().tolist() == [0, 0, 0]
    if name == "path130":
        assert rounds.cpu().tolist() == [65]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["w16_ties", "w3_nonfinite", "lds_plus_one"])
def test_same_bits_whatever_the_buffers_held(dev, monkeypatch, name, form):
    """Two runs, and runs over poisoned outputs and a poisoned workspace, give the same bits."""
    from deepmetv2_amd import _native
    _form(monkeypatch, form)
    args = _native_args(CASES[name], dev)
    first = _native._edge_match(*args, want_rounds=True)
    again = _native._edge_match(*args, want_rounds=True)
    got = run_both(lambda: _native._edge_match(*args, want_rounds=True))
    for i, a in enumerate(first):
        assert _same(a, again[i])
        for pattern in got:
            assert _same(a.cpu(), got[pattern][i]), (pattern, i)


@pytest.mark.parametrize("name", ["w3_distinct", "w16_distinct"])
def test_a_shuffled_edge_order_gives_the_same_clusters(dev, rule, name):
    import deepmetv2_amd as dm
    case = CASES[name]
    batch = _batch(dev, case.sizes)
    g = torch.Generator().manual_seed(3)
    ei, score = torch.from_numpy(case.edge_index), torch.from_numpy(case.score)
    # the duplicate edges of these cases carry distinct scores; give every edge its own so that no tie is broken by position
    score = torch.randperm(score.numel(), generator=g).float()
    base, base_edge = dm.edge_matching(ei.to(dev), score.to(dev), batch)
    want = er.sequential_match(ei[0], ei[1], score.numpy(), np.arange(ei.shape[1]), er.ptr_of(case.sizes), batch.numel())
    assert torch.equal(base.cpu(), torch.from_numpy(want[0])) and torch.equal(base_edge.cpu(), torch.from_numpy(want[2]))
    for _ in range(2):
        p = torch.randperm(ei.shape[1], generator=g)
        cluster, edge = dm.edge_matching(ei[:, p].contiguous().to(dev), score[p].to(dev), batch)
        assert torch.equal(cluster, base)
        claimed = edge.cpu() >= 0
        assert torch.equal(p[edge.cpu()[claimed]], base_edge.cpu()[claimed])         # the same edges, by their new positions


def test_bad_edges_are_reported_later_and_change_nothing_else(dev, rule):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native, edge_pool
    from deepmetv2_amd.graph import EdgeList
    want = rule["w3_distinct"]
    for name, case, flag in er.bad_edge_cases():
        rowptr, src, tgt, perm, score, ptr = _native_args(case, dev)
        cluster, partner, edge, _r, flags = _native._edge_match(rowptr, src, tgt, perm, score, ptr)
        assert torch.equal(cluster.cpu(), torch.from_numpy(want[0])) and torch.equal(edge.cpu(), torch.from_numpy(want[2]))
        assert torch.equal(partner.cpu().long(), torch.from_numpy(want[1]))
        assert flags.cpu().tolist() == [int(flag == 0), int(flag == 1), 0], name
        # the same through the package's own launch path: nothing raises at the call, the next drain does
        g = edge_pool._Grouped(EdgeList(src.clamp(0, sum(case.sizes) - 1), tgt, rowptr, sum(case.sizes), perm), src)
        cluster2, _p, _e, _r = edge_pool._match(g, score, ptr, "edge_matching")
        assert torch.equal(cluster2, cluster)
        with pytest.raises(RuntimeError, match="two events" if flag == 1 else r"outside \[0, 166\)"):
            dm.raise_deferred_errors()
    name, case, _flag = er.bad_edge_cases()[0]
    batch = _batch(dev, case.sizes)
    cluster, _edge = dm.edge_matching(torch.from_numpy(case.edge_index).to(dev), torch.from_numpy(case.score).to(dev), batch)
    assert torch.equal(cluster.cpu(), torch.from_numpy(want[0]))
    with pytest.raises(RuntimeError, match="edge_matching: an edge joins nodes of two events"):
        dm.raise_deferred_errors()


def test_empty_inputs(dev):
    import deepmetv2_amd as dm
    none = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    z = torch.zeros(0, device=dev)
    cluster, edge, rounds = dm.edge_matching(none, z, _batch(dev, [3, 0, 2]), return_rounds=True)
    assert cluster.tolist() == [0, 1, 2, 3, 4] and edge.tolist() == [-1] * 5 and rounds.tolist() == [0, 0, 0]
    cluster, edge = dm.edge_matching(none, z, num_nodes=0)
    assert cluster.numel() == 0 and edge.numel() == 0
    cluster, edge = dm.edge_matching(none, z, num_nodes=4)                 # no batch: one event without edges
    assert cluster.tolist() == [0, 1, 2, 3] and edge.tolist() == [-1] * 4


def _count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return sum("called a synchronizing" in str(r.message) for r in rec)


def test_a_knn_graph_keeps_its_grouping_and_costs_no_host_read(dev):
    """edge_matching over a knn_graph tensor with a registered batch: the rule's result, pooled through the pair route, and
    no device-to-host sync in the call."""
    import deepmetv2_amd as dm
    sizes = [40, 7, 90]
    batch = _batch(dev, sizes)
    g = torch.Generator().manual_seed(8)
    pos = torch.randn(sum(sizes), 2, generator=g)
    ei = dm.knn_graph(pos.to(dev), 6, batch)
    score = torch.rand(ei.shape[1], generator=g)
    sd = score.to(dev)
    dm.edge_matching(ei, sd, batch)                         # warm-up (library, workspaces)
    got = {}
    assert _count_syncs(lambda: got.update(r=dm.edge_matching(ei, sd, batch))) == 0
    cluster, edge = got["r"]
    e = ei.cpu()
    want = er.sequential_match(e[0], e[1], score.numpy(), np.arange(e.shape[1]), er.ptr_of(sizes), sum(sizes))
    assert torch.equal(cluster.cpu(), torch.from_numpy(want[0])) and torch.equal(edge.cpu(), torch.from_numpy(want[2]))
    x = torch.randn(sum(sizes), 4, generator=g).to(dev)
    out, pooled = dm.max_pool_x(cluster, x, batch)
    cid, leaders = er.pooled_rows(want[0])
    ref = torch.full((len(leaders), 4), float("-inf")).scatter_reduce(0, torch.from_numpy(cid).view(-1, 1).expand(-1, 4),
                                                                      x.cpu(), "amax")
    assert torch.equal(out.cpu(), ref) and torch.equal(pooled.cpu(), batch.cpu()[torch.from_numpy(leaders)])


# ---- the layer ------------------------------------------------------------------------------------------------------------------
def _layer(dev, method, add, w, b):
    import deepmetv2_amd as dm
    pool = dm.EdgePooling(er.LAYER_F, getattr(dm.EdgePooling, "compute_edge_score_" + method), add_to_edge_score=add)
    with torch.no_grad():
        pool.lin.weight.copy_(w)
        pool.lin.bias.copy_(b)
    return pool.to(dev)


def _hold(got, want, cpu32, what):
    for name in want:
        a, b, c = got[name].cpu().double(), want[name], cpu32[name].double()
        scale = float(b.abs().max())
        err, base = float((a - b).abs().max()), float((c - b).abs().max())
        tol = 4 * base + 1e-6 * scale
        print(f"{what} {name}: error {err:.2e}, fp32 torch composition on the CPU {base:.2e}, tolerance {tol:.2e}, "
              f"ratio {err / max(tol, 1e-300):.3f}")
    for name in want:
        a, b, c = got[name].cpu().double(), want[name], cpu32[name].double()
        tol = 4 * float((c - b).abs().max()) + 1e-6 * float(b.abs().max())
        assert float((a - b).abs().max()) <= tol, (what, name)


@pytest.mark.parametrize("name,case,method,add", er.layer_cases(), ids=[c[0] for c in er.layer_cases()])
def test_layer_against_the_rule_and_its_float64_restatement(dev, name, case, method, add):
    """Measured on an MI355X, the largest error / tolerance ratio over scores, new_edge_score, new_x and the gradients to x,
    lin.weight and lin.bias: w3_softmax 0.10, w16_softmax 0.12, w16_tanh 0.14, w3_sigmoid 0.17.  The fp32 torch composition's
    own errors, which set the tolerances, are between 3e-8 and 5e-6 in absolute terms on these tensors (the printed lines)."""
    from deepmetv2_amd.graph import _batch_registry, _registry_get
    x, w, b, g = er.layer_inputs(case)
    ei = torch.from_numpy(case.edge_index)
    N, ptr = x.shape[0], er.ptr_of(case.sizes)
    batch = _batch(dev, case.sizes)
    pool = _layer(dev, method, add, w, b)
    xd, eid = x.to(dev).requires_grad_(True), ei.to(dev)
    scores = pool.scores(xd, eid, batch)
    new_x, new_ei, new_batch, info = pool(xd, eid, batch)
    # the partition: the sequential rule on the scores the layer itself returned
    cluster, _p, edge = er.sequential_match(ei[0], ei[1], scores.detach().cpu().numpy(), np.arange(ei.shape[1]), ptr, N)
    cid, leaders = er.pooled_rows(cluster)
    assert torch.equal(info.cluster.cpu(), torch.from_numpy(cid))
    assert new_x.shape == (len(leaders), er.LAYER_F)
    # what follows from the partition exactly
    assert torch.equal(new_ei.cpu(), torch.from_numpy(er.coalesced(cid, case.edge_index)))
    nb = new_batch.cpu()
    assert bool((nb[1:] >= nb[:-1]).all()) and torch.equal(nb, batch.cpu()[torch.from_numpy(leaders)])
    assert _registry_get(_batch_registry, new_batch) is not None
    (new_x * g[:len(leaders)].to(dev)).sum().backward()
    got = {"scores": scores.detach(), "new_edge_score": info.new_edge_score.detach(), "new_x": new_x.detach(),
           "g_x": xd.grad, "g_weight": pool.lin.weight.grad, "g_bias": pool.lin.bias.grad}
    want = dict(er.layer_tensors(torch.float64, x, ei, w, b, method, add, cluster, edge, g[:len(leaders)]))
    cpu32 = dict(er.layer_tensors(torch.float32, x, ei, w, b, method, add, cluster, edge, g[:len(leaders)]))
    _hold(got, want, cpu32, name)
    # the same bits again, gradients included
    x2 = x.to(dev).requires_grad_(True)
    pool.zero_grad()
    again = pool(x2, eid, batch)[0]
    (again * g[:len(leaders)].to(dev)).sum().backward()
    assert _same(again, new_x) and _same(x2.grad, xd.grad) and _same(pool.lin.weight.grad, got["g_weight"])
    ux, _uei, _ub = pool.unpool(new_x.detach(), info)
    assert ux.shape == x.shape


def test_unit_scores_give_the_pair_sums_bit_for_bit(dev):
    """lin = 0 and tanh with add_to_edge_score = 1: every score is exactly 1, ties everywhere go to the lower edge id, and
    new_x is fl(x_u + x_v) for a pair, x_u for a one-node cluster."""
    case = er.mixed_cases()[1]
    x, w, b, _g = er.layer_inputs(case)
    ei = torch.from_numpy(case.edge_index)
    N = x.shape[0]
    batch = _batch(dev, case.sizes)
    pool = _layer(dev, "tanh", 1.0, torch.zeros_like(w), torch.zeros_like(b))
    new_x, _ei, _nb, info = pool(x.to(dev), ei.to(dev), batch)
    assert bool((pool.scores(x.to(dev), ei.to(dev), batch) == 1).all()) and bool((info.new_edge_score == 1).all())
    cluster, partner, _e = er.sequential_match(ei[0], ei[1], np.ones(ei.shape[1], np.float32), np.arange(ei.shape[1]),
                                               er.ptr_of(case.sizes), N)
    cid, leaders = er.pooled_rows(cluster)
    assert torch.equal(info.cluster.cpu(), torch.from_numpy(cid))
    mate = torch.from_numpy(partner[leaders])
    xl = x[torch.from_numpy(leaders)]
    sums = torch.where((mate >= 0).view(-1, 1), xl + x[mate.clamp(min=0)], xl)
    assert _same(new_x.cpu(), sums)


def test_forward_host_reads(dev):
    """With a registered batch and a knn_graph tensor: the pooled sizes (one read) and whatever torch.unique costs for the
    coalesced edge count; nothing else."""
    import deepmetv2_amd as dm
    sizes = [40, 7, 90]
    batch = _batch(dev, sizes)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(sum(sizes), er.LAYER_F, generator=g).to(dev)
    ei = dm.knn_graph(x[:, :2].contiguous(), 6, batch)
    pool = dm.EdgePooling(er.LAYER_F).to(dev)
    out = pool(x, ei, batch)                                # warm-up
    key = out[3].cluster[ei[0]] * out[0].shape[0] + out[3].cluster[ei[1]]
    unique = _count_syncs(lambda: torch.unique(key, sorted=True, return_inverse=True))
    n = _count_syncs(lambda: pool(x, ei, batch))
    print(f"EdgePooling.forward: {n} host reads, {unique} of them torch.unique's")
    assert n == 1 + unique

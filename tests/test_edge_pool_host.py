"""Edge pooling without a GPU: the round rule against the sequential rule, the conditions that keep the GPU tests of
tests/test_gpu_edge_pool.py from passing on nothing, and the host logic of deepmetv2_amd/edge_pool.py over CPU stand-ins."""
import numpy as np
import pytest
import torch

import edge_pool_reference as er

CASES = {c.name: c for c in er.all_cases()}
CASES.update({name: c for name, c, _flag in er.bad_edge_cases()})


def _run(case, rule):
    N = sum(case.sizes)
    return rule(case.edge_index[0], case.edge_index[1], case.score, np.arange(case.edge_index.shape[1]),
                er.ptr_of(case.sizes), N)


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def test_the_order_is_the_canonical_one():
    v = np.array([np.nan, -np.nan, np.inf, 3e38, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -np.inf], np.float32)
    hi = er.order_bits(v)
    assert hi[0] == hi[1] == 0xFFFFFFFF and hi[6] == hi[7]
    assert list(hi[1:7]) == sorted(hi[1:7], reverse=True) and len(set(hi[1:7])) == 6
    assert list(hi[7:]) == sorted(hi[7:], reverse=True) and len(set(hi[7:])) == 4
    k = er.keys(np.array([1.0, 1.0], np.float32), [3, 4])
    assert k[0] > k[1] and int(er.keys(np.array([-np.inf], np.float32), [2 ** 31 - 1])[0]) > 1       # above both state words


@pytest.mark.parametrize("name", list(CASES))
def test_rounds_take_the_edges_of_the_sequential_rule(name):
    case = CASES[name]
    want = _run(case, er.sequential_match)
    cluster, partner, edge, rounds, flags = _run(case, er.round_match)
    for a, b in zip(want, (cluster, partner, edge)):
        assert np.array_equal(a, b)
    assert flags[2] == 0 and len(rounds) == len(case.sizes)


@pytest.mark.parametrize("case", er.mixed_cases(), ids=lambda c: c.name)
def test_mixed_cases_show_every_kind_of_node(case):
    cluster, partner, edge = _run(case, er.sequential_match)
    assert int((partner >= 0).sum()) >= 2                                   # a pair
    assert int(((partner < 0) & (edge >= 0)).sum()) >= 1                    # a self-loop singleton
    assert int((edge < 0).sum()) >= 2                                       # unclaimed nodes
    ptr = er.ptr_of(case.sizes)
    a = int(ptr[er.RAGGED.index(2)])
    assert partner[a] == -1 and edge[a] >= 0 and edge[a + 1] == -1 and edge[int(ptr[er.RAGGED.index(1)])] == -1
    ei = case.edge_index
    assert np.array_equal(np.sort(ei[1]), ei[1]) is False                   # arrives ungrouped
    pairs = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert len(pairs) < ei.shape[1] and any((t, s) in pairs for s, t in pairs if s != t) and any(s == t for s, t in pairs)
    assert _run(case, er.round_match)[3].max() >= 3


def test_ties_and_non_finite_scores_are_there():
    ties, odd = er.mixed_cases()[2], er.mixed_cases()[3]
    assert set(np.unique(ties.score)) == {1.0, 2.0, 3.0}
    s = odd.score
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any()
    assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any()


def test_the_path_runs_65_rounds_and_the_large_event_passes_the_lds_limit():
    path = er.path_case()
    cluster, partner, edge, rounds, _flags = _run(path, er.round_match)
    assert rounds.tolist() == [65] and int((partner >= 0).sum()) == 130
    assert np.array_equal(edge[::2], np.arange(0, 129, 2)) and np.all(np.diff(path.score) < 0)
    big = er.big_case()
    assert big.sizes == [er.LDS_NODES + 1] and big.edge_index.shape[1] == 3 * (er.LDS_NODES + 1)
    assert _run(big, er.round_match)[3][0] >= 3


def test_bad_edges_change_nothing_else():
    base = _run(er.mixed_cases()[0], er.sequential_match)
    for name, case, flag in er.bad_edge_cases():
        got = _run(case, er.round_match)
        for a, b in zip(base, got[:3]):
            assert np.array_equal(a, b), name
        assert got[4][flag] == 1 and got[4].sum() == 1, name


# ---- the layer's restatements ----------------------------------------------------------------------------------------------------
def _leaders_of(upstream_cluster):
    """cluster[N] in graclus's convention (the lowest member) from upstream's cluster numbers."""
    c = np.asarray(upstream_cluster)
    low = np.full(int(c.max()) + 1, len(c), np.int64)
    np.minimum.at(low, c, np.arange(len(c)))
    return low[c]


@pytest.mark.parametrize("name,case,method,add", er.layer_cases(), ids=[c[0] for c in er.layer_cases()])
def test_fp32_and_float64_scores_choose_one_partition(name, case, method, add):
    """So that no tolerance of the GPU test is asked to cover a flipped match on these inputs."""
    x, w, b, _g = er.layer_inputs(case)
    ei = torch.from_numpy(case.edge_index)
    N, ptr = x.shape[0], er.ptr_of(case.sizes)
    e32 = er.edge_scores(x, ei, w, b, method, add)
    e64 = er.edge_scores(x.double(), ei, w.double(), b.double(), method, add)
    c32, _p, _e = er.sequential_match(ei[0], ei[1], e32.numpy(), np.arange(ei.shape[1]), ptr, N)
    up, _taken = er.upstream_merge(e64.numpy(), case.edge_index, N)
    assert np.array_equal(c32, _leaders_of(up))


@pytest.mark.parametrize("name,case,method,add", er.layer_cases(), ids=[c[0] for c in er.layer_cases()])
def test_the_restatement_on_a_partition_is_upstreams_forward_relabelled(name, case, method, add):
    x, w, b, g = er.layer_inputs(case)
    ei = torch.from_numpy(case.edge_index)
    N = x.shape[0]
    new_x, new_ei, up, score = er.upstream_forward(x.double(), ei, w.double(), b.double(), method, add)
    e64 = er.edge_scores(x.double(), ei, w.double(), b.double(), method, add)
    # events do not matter to upstream's walk as long as no edge crosses them
    cluster, _p, edge = er.sequential_match(ei[0], ei[1], e64.float().numpy(), np.arange(ei.shape[1]), er.ptr_of(case.sizes), N)
    assert np.array_equal(cluster, _leaders_of(up.numpy()))
    cid, leaders = er.pooled_rows(cluster)
    relabel = up.numpy()[leaders]                           # my row -> upstream's row
    got = dict(er.layer_tensors(torch.float64, x, ei, w, b, method, add, cluster, edge, g[:len(leaders)]))
    assert torch.equal(got["new_x"], new_x[relabel]) and torch.equal(got["new_edge_score"], score[relabel])
    back = np.empty_like(relabel)
    back[relabel] = np.arange(len(relabel))
    mine = er.coalesced(cid, case.edge_index)
    theirs = back[new_ei.numpy()]
    order = np.lexsort((theirs[1], theirs[0]))
    assert np.array_equal(mine, theirs[:, order])
    assert torch.equal(er.upstream_unpool(new_x, up, score), (got["new_x"] / got["new_edge_score"].view(-1, 1))[cid])


# ---- host logic over the stand-ins -------------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    return er.FakeNative().install(monkeypatch)


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64))


def test_argument_errors(fake):
    import deepmetv2_amd as dm
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    s = torch.tensor([0.3, 0.2, 0.1])
    with pytest.raises(ValueError, match="edge_index"):
        dm.edge_matching(ei.t(), s, num_nodes=3)
    with pytest.raises(TypeError, match="int64"):
        dm.edge_matching(ei.int(), s, num_nodes=3)
    with pytest.raises(TypeError, match="float64"):
        dm.edge_matching(ei, s.double(), num_nodes=3)
    with pytest.raises(TypeError, match="floating-point"):
        dm.edge_matching(ei, torch.tensor([3, 2, 1]), num_nodes=3)
    with pytest.raises(ValueError, match=r"\[3\]"):
        dm.edge_matching(ei, s[:2], num_nodes=3)
    with pytest.raises(ValueError, match="sorted"):
        dm.edge_matching(ei, s, torch.tensor([1, 0, 1]))
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        dm.edge_matching(torch.tensor([[0, 5], [1, 2]]), s[:2], num_nodes=3)
    pool = dm.EdgePooling(4)
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        pool(torch.zeros(3, 5), ei)
    with pytest.raises(TypeError, match="float32"):
        pool(torch.zeros(3, 4, dtype=torch.float64), ei)
    with pytest.raises(TypeError, match="callable"):
        dm.EdgePooling(4, edge_score_method="tanh")
    assert fake.calls == {}


@pytest.mark.parametrize("case", er.mixed_cases(), ids=lambda c: c.name)
def test_edge_matching_over_the_stand_in(fake, case):
    """The grouping, the permutation of the scores along with it, caller-order edge ids, bf16 scores, the registration."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import pool as dpool
    from deepmetv2_amd.graph import _registry_get
    ei, batch = torch.from_numpy(case.edge_index), _batch(case.sizes)
    want = _run(case, er.sequential_match)
    cluster, edge, rounds = dm.edge_matching(ei, torch.from_numpy(case.score), batch, return_rounds=True)
    assert torch.equal(cluster, torch.from_numpy(want[0])) and torch.equal(edge, torch.from_numpy(want[2]))
    assert cluster.dtype == edge.dtype == torch.int64 and rounds.dtype == torch.int32 and rounds.numel() == len(case.sizes)
    partner = _registry_get(dpool._graclus_registry, cluster)
    assert partner is not None and torch.equal(partner.long(), torch.from_numpy(want[1]))
    x = torch.randn(batch.numel(), 3)
    out, pooled_batch = dm.max_pool_x(cluster, x, batch)
    assert fake.calls.get("pool_pairs") == 1 and out.shape[0] == len(np.unique(want[0]))
    assert bool((pooled_batch[1:] >= pooled_batch[:-1]).all())
    half = torch.from_numpy(case.score).to(torch.bfloat16)
    c16, _e16 = dm.edge_matching(ei, half, batch)
    w16 = er.sequential_match(ei[0], ei[1], half.float().numpy(), np.arange(ei.shape[1]), er.ptr_of(case.sizes), batch.numel())
    assert torch.equal(c16, torch.from_numpy(w16[0]))


def test_empty_inputs_over_the_stand_in(fake):
    import deepmetv2_amd as dm
    none = torch.zeros((2, 0), dtype=torch.int64)
    cluster, edge = dm.edge_matching(none, torch.zeros(0), _batch([3, 0, 2]))
    assert cluster.tolist() == [0, 1, 2, 3, 4] and edge.tolist() == [-1] * 5
    cluster, edge = dm.edge_matching(none, torch.zeros(0), num_nodes=0)
    assert cluster.numel() == 0 and edge.numel() == 0


def _hold(got, want, cpu32, what):
    for name in want:
        a, b, c = got[name].double(), want[name], cpu32[name].double()
        tol = 4 * float((c - b).abs().max()) + 1e-6 * float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"{what} {name}: error {err:.2e}, tolerance {tol:.2e}")
        assert err <= tol, (what, name, err, tol)


@pytest.mark.parametrize("name,case,method,add", er.layer_cases(), ids=[c[0] for c in er.layer_cases()])
def test_layer_over_the_stand_ins(fake, name, case, method, add):
    """The plumbing: the split of lin.weight, the grouped softmax, the leader gathers, the coarsened edges, unpool."""
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import _batch_registry, _registry_get
    x, w, b, g = er.layer_inputs(case)
    ei, batch = torch.from_numpy(case.edge_index), _batch(case.sizes)
    N, ptr = x.shape[0], er.ptr_of(case.sizes)
    pool = dm.EdgePooling(er.LAYER_F, getattr(dm.EdgePooling, "compute_edge_score_" + method), add_to_edge_score=add)
    assert sorted(pool.state_dict()) == ["lin.bias", "lin.weight"] and pool.lin.weight.shape == (1, 2 * er.LAYER_F)
    with torch.no_grad():
        pool.lin.weight.copy_(w)
        pool.lin.bias.copy_(b)
    xr = x.clone().requires_grad_(True)
    scores = pool.scores(xr, ei, batch)
    new_x, new_ei, new_batch, info = pool(xr, ei, batch)
    cluster, _p, edge = er.sequential_match(ei[0], ei[1], scores.detach().numpy(), np.arange(ei.shape[1]), ptr, N)
    cid, leaders = er.pooled_rows(cluster)
    assert torch.equal(info.cluster, torch.from_numpy(cid)) and new_x.shape == (len(leaders), er.LAYER_F)
    assert torch.equal(new_ei, torch.from_numpy(er.coalesced(cid, case.edge_index)))
    assert _registry_get(_batch_registry, new_batch) is not None and bool((new_batch[1:] >= new_batch[:-1]).all())
    assert torch.equal(new_batch, batch[torch.from_numpy(leaders)])
    (new_x * g[:len(leaders)]).sum().backward()
    got = {"scores": scores.detach(), "new_edge_score": info.new_edge_score.detach(), "new_x": new_x.detach(),
           "g_x": xr.grad, "g_weight": pool.lin.weight.grad, "g_bias": pool.lin.bias.grad}
    want = dict(er.layer_tensors(torch.float64, x, ei, w, b, method, add, cluster, edge, g[:len(leaders)]))
    cpu32 = dict(er.layer_tensors(torch.float32, x, ei, w, b, method, add, cluster, edge, g[:len(leaders)]))
    _hold(got, want, cpu32, name)
    ux, uei, ub = pool.unpool(new_x.detach(), info)
    assert ux.shape == x.shape and uei is ei and ub is batch
    sums = torch.zeros(len(leaders), er.LAYER_F).index_add(0, info.cluster, x)
    torch.testing.assert_close(ux, sums[info.cluster], rtol=1e-5, atol=1e-6)        # x up to the divide: the member sums


def test_a_callers_score_method_sees_the_callers_order(fake):
    import deepmetv2_amd as dm
    case = er.mixed_cases()[0]
    x, w, b, _g = er.layer_inputs(case)
    ei, batch = torch.from_numpy(case.edge_index), _batch(case.sizes)
    seen = {}

    def method(raw, edge_index, num_nodes):
        seen["args"] = (raw.detach().clone(), edge_index, num_nodes)
        return torch.tanh(raw)

    pool = dm.EdgePooling(er.LAYER_F, method, add_to_edge_score=0.25)
    with torch.no_grad():
        pool.lin.weight.copy_(w)
        pool.lin.bias.copy_(b)
    s = pool.scores(x, ei, batch)
    raw = torch.nn.functional.linear(torch.cat([x[ei[0]], x[ei[1]]], -1), w, b).view(-1)
    assert seen["args"][1] is ei and seen["args"][2] == x.shape[0]
    torch.testing.assert_close(seen["args"][0], raw, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(s, torch.tanh(raw) + 0.25, rtol=1e-5, atol=1e-6)


def test_exports_and_pool_edge_default():
    import deepmetv2_amd as dm
    from deepmetv2_amd import pool as dpool
    assert {"EdgePooling", "edge_matching"} <= set(dm.__all__)
    assert "EdgePooling" in dm.__doc__ and "edge_matching" in dm.__doc__
    node_map = torch.tensor([0, 0, 1, 2, 2])
    ei = torch.tensor([[0, 1, 2, 3, 4, 2, 0], [1, 2, 3, 4, 0, 3, 0]])
    today, _attr = dpool.pool_edge(node_map, ei, None, 3)
    assert today.tolist() == [[0, 1, 2], [1, 2, 0]]                                 # self loops dropped, coalesced: as it was
    kept, _attr = dpool.pool_edge(node_map, ei, None, 3, self_loops=True)
    assert torch.equal(kept, torch.from_numpy(er.coalesced(node_map.numpy(), ei.numpy())))
    assert kept.tolist() == [[0, 0, 1, 2, 2], [0, 1, 2, 0, 2]]

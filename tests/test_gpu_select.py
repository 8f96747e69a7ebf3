"""csrc/select.hip and deepmetv2_amd/select.py on the GPU against tests/select_reference.py.

One ragged batch (sr.LENGTHS: an empty event first and last, the wave and workgroup edges, both sides of a power of two,
T - 1, T, T + 1 around the LDS route's limit T = DMET_SELECT_LDS_NODES and T + 3000 on the workspace route), four kinds
of score (Gaussian, ties from {-1, 0, 1}, all equal, and +-0.0 / +-inf / +-NaN seeded into a Gaussian).

Held exactly: perm and node_map (-1 slots included), filter_table, filter_adj with `kept`, select_rows forward and gx (one
multiply each: the bits of the fp32 restatement).  gs is held against float64 within gamma_F sum_f |g x| per node
(gamma_n = n u / (1 - n u), u = 2^-24: one rounding per product, F - 1 additions, any order).  Every operator returns the
same bits under both poison patterns.

The layers: perm must equal the reference ranking of the layer's own scores(...); scores and the outputs given that perm
are held to the float64 restatement within, per tensor, 4 times the largest error of the same formula composed from fp32
torch operators on the CPU against float64.  Every such check prints its error / bound ratio before it asserts.
"""
import pytest
import torch

import poisoned_alloc as pa
import select_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    """The tests of this file seed and draw from torch's global generators; what later tests find there stays as it was."""
    with torch.random.fork_rng(devices=[0] if torch.cuda.is_available() else []):
        yield


def _hold(what, got, want, lim):
    err = (got.detach().cpu().double() - want).abs()
    lim = torch.as_tensor(lim, dtype=torch.float64).expand_as(err)
    ratio = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max err/bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= lim).all()), (what, ratio)


def _same_bits(a, b):
    return pa.differing(a.cpu(), b.cpu()).numel() == 0


class _NoSync:
    """Any synchronising call of torch on the device raises inside the block (after the caller's warm-up)."""

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


def _register(lengths, dev):
    from deepmetv2_amd import register_batch
    batch = sr.batch_of(lengths).to(dev)
    register_batch(batch, sr.ptr_of(lengths).to(dev), len(lengths), max_nodes=max(lengths), min_nodes=min(lengths))
    return batch


# ---- 1. topk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", sr.RATIOS)
@pytest.mark.parametrize("kind", sr.KINDS)
def test_topk_equals_the_reference_ranking(dev, kind, ratio):
    from deepmetv2_amd import topk
    s = sr.scores(kind)
    want_perm, want_map, _ = sr.topk_ratio(s, sr.LENGTHS, ratio, orders=sr.orders_of(kind))
    perm, node_map = topk(s.to(dev), ratio, ptr=sr.ptr_of(sr.LENGTHS).to(dev), return_map=True)
    assert perm.dtype == torch.int64 and node_map.dtype == torch.int32
    assert torch.equal(perm.cpu(), want_perm) and torch.equal(node_map.cpu(), want_map)
    again = topk(s.to(dev), ratio, _register(sr.LENGTHS, dev))
    assert torch.equal(again, perm)


@pytest.mark.parametrize("kind", sr.KINDS)
def test_topk_slot_ranges_longer_than_events_end_in_minus_one(dev, kind):
    """Slot ranges of 70 per event (the sort-pool form): shorter events fill up with -1, nothing lands beyond perm[M]."""
    from deepmetv2_amd import _native
    s, ptr, B = sr.scores(kind), sr.ptr_of(sr.LENGTHS), len(sr.LENGTHS)
    out_ptr = torch.arange(B + 1) * 70
    want_perm, want_map = sr.topk(s, ptr, out_ptr, 70 * B, orders=sr.orders_of(kind))
    res = pa.run_both(lambda: _native._topk(s.to(dev), ptr.to(dev), out_ptr.to(dev), 70 * B))
    for pattern in pa.PATTERNS:
        assert torch.equal(res[pattern][0], want_perm) and torch.equal(res[pattern][1], want_map), pattern
    assert int((want_perm == -1).sum()) > 0 and int((want_perm == -7).sum()) == 0
    # a perm cut short: M below out_ptr[B]
    M = 70 * 5 + 13
    cut_perm, cut_map = _native._topk(s.to(dev), ptr.to(dev), out_ptr.to(dev), M)
    ref_perm, ref_map = sr.topk(s, ptr, out_ptr.clamp(max=M), M, orders=sr.orders_of(kind))
    assert torch.equal(cut_perm.cpu(), ref_perm) and torch.equal(cut_map.cpu(), ref_map)


def test_topk_same_bits_under_both_poison_patterns(dev):
    from deepmetv2_amd import topk
    s = sr.scores("special").to(dev)
    ptr = sr.ptr_of(sr.LENGTHS).to(dev)
    res = pa.run_both(lambda: topk(s, 0.5, ptr=ptr, return_map=True))
    for a, b in zip(res["ones"], res["zeros_huge"]):
        assert torch.equal(a, b)


# ---- 2. filter_table ------------------------------------------------------------------------------------------------------------
def _table_case(k, counted, seed=0):
    g = torch.Generator().manual_seed(40 + k + seed)
    lengths = [0, 70, 1, 130, 257]
    N = sum(lengths)
    s = torch.randn(N, generator=g)
    perm, node_map, out_ptr = sr.topk_ratio(s, lengths, 0.5)
    nbr = torch.randint(0, N, (N, k), generator=g).to(torch.int32)
    nbr[torch.rand(N, k, generator=g) < 0.25] = -1                      # holes
    nbr[torch.arange(N), torch.randint(0, k, (N,), generator=g)] = torch.arange(N, dtype=torch.int32)     # self entries
    picked, unpicked = (node_map >= 0).nonzero().view(-1), (node_map < 0).nonzero().view(-1)
    all_row, none_row = int(perm[3]), int(perm[-2])
    nbr[all_row] = picked[torch.randint(0, picked.numel(), (k,), generator=g)].to(torch.int32)       # keeps everything
    nbr[none_row] = unpicked[torch.randint(0, unpicked.numel(), (k,), generator=g)].to(torch.int32)  # keeps nothing
    cnt = None
    if counted:
        cnt = torch.randint(0, k + 1, (N,), generator=g).to(torch.int32)
        cnt[all_row] = k
        cnt[none_row] = k
    perm = torch.cat([perm, torch.tensor([-1])])                          # and a row that selects no node
    return nbr, cnt, perm, node_map, 3, perm.numel() - 3


@pytest.mark.parametrize("k,counted", [(1, False), (16, False), (20, False), (64, False), (255, True), (1024, True)])
def test_filter_table_equals_its_restatement(dev, k, counted):
    from deepmetv2_amd import _native
    nbr, cnt, perm, node_map, all_r, none_r = _table_case(k, counted)
    want_nbr, want_cnt = sr.filter_table(nbr, cnt, perm, node_map)
    res = pa.run_both(lambda: _native._filter_table(nbr.to(dev), None if cnt is None else cnt.to(dev), perm.to(dev),
                                                   node_map.to(dev)))
    for pattern in pa.PATTERNS:
        got_nbr, got_cnt = res[pattern]
        assert torch.equal(got_nbr, want_nbr) and torch.equal(got_cnt, want_cnt), pattern
    slot = torch.arange(k).view(1, -1)
    assert bool((got_nbr[slot >= got_cnt.view(-1, 1)] == -1).all()) and bool((got_nbr[slot < got_cnt.view(-1, 1)] >= 0).all())
    assert int(got_cnt[all_r]) == k and int(got_cnt[none_r]) == 0 and int(got_cnt[-1]) == 0


# ---- 3. filter_adj --------------------------------------------------------------------------------------------------------------
def _edge_case(E, seed=0):
    g = torch.Generator().manual_seed(60 + seed)
    lengths = [0, 70, 1, 130, 257]
    N = sum(lengths)
    perm, node_map, _ = sr.topk_ratio(torch.randn(N, generator=g), lengths, 0.5)
    ei = torch.randint(0, N, (2, E), generator=g)
    if E > 10:
        ei[:, 5] = ei[:, 2]                         # a duplicate
        ei[1, 7] = ei[0, 7] = int(perm[0])          # a kept self loop
        ei[:, E // 2:] = ei[:, E // 2:].flip(1)     # no order
    return ei, perm, node_map, N


@pytest.mark.parametrize("E", [0, 1, 1024, 5000])
def test_filter_adj_equals_its_restatement(dev, E):
    from deepmetv2_amd import filter_adj, raise_deferred_errors
    ei, perm, node_map, N = _edge_case(E)
    if E == 1:
        ei[:, 0] = perm[:2]                         # the one edge is kept
    attr = torch.randn(E, 3)
    want_ei, want_kept, _ = sr.filter_edges(ei, node_map)
    res = pa.run_both(lambda: filter_adj(ei.to(dev), attr.to(dev), perm.to(dev), N, node_map=node_map.to(dev))) if E else None
    got_ei, got_attr = filter_adj(ei.to(dev), attr.to(dev), perm.to(dev), N, node_map=node_map.to(dev))
    assert torch.equal(got_ei.cpu(), want_ei) and torch.equal(got_attr.cpu(), attr[want_kept]) and got_ei.dtype == torch.int64
    if E:
        for pattern in pa.PATTERNS:
            assert torch.equal(res[pattern][0], want_ei) and torch.equal(res[pattern][1], attr[want_kept]), pattern
        assert E == 1 or 0 < want_ei.shape[1] < E
    by_scatter, _ = filter_adj(ei.to(dev), None, perm.to(dev), N)       # the inverse built by one scatter
    assert torch.equal(by_scatter.cpu(), want_ei)
    raise_deferred_errors()


def test_filter_edges_returns_kept_and_drops_an_out_of_range_id(dev):
    from deepmetv2_amd import _native, filter_adj, raise_deferred_errors
    ei, perm, node_map, N = _edge_case(5000, seed=1)
    raise_deferred_errors()
    out, kept, nbad = _native._filter_edges(ei.to(dev), node_map.to(dev))
    want_ei, want_kept, _ = sr.filter_edges(ei, node_map)
    assert torch.equal(kept.cpu(), want_kept) and torch.equal(out.cpu(), want_ei) and int(nbad) == 0
    bad = ei.clone()
    bad[0, 3000] = N                                # one id out of range, at an edge that would otherwise be kept or not
    bad[1, 3000] = int(perm[0])
    want_ei, want_kept, nb = sr.filter_edges(bad, node_map)
    got, _ = filter_adj(bad.to(dev), None, perm.to(dev), N, node_map=node_map.to(dev))
    assert nb == 1 and torch.equal(got.cpu(), want_ei) and 3000 not in want_kept.tolist()
    with pytest.raises(RuntimeError, match="filter_adj"):
        raise_deferred_errors()
    neg = ei.clone()
    neg[1, 17] = -1
    out, kept, nbad = _native._filter_edges(neg.to(dev), node_map.to(dev))
    assert int(nbad) == 1 and torch.equal(out.cpu(), sr.filter_edges(neg, node_map)[0])


# ---- 4. select_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 64, 65, 300])
def test_select_rows_and_its_backward(dev, F):
    from deepmetv2_amd import _native
    g0 = torch.Generator().manual_seed(80 + F)
    lengths = [0, 70, 1, 130, 257]
    N = sum(lengths)
    out_ptr = torch.arange(len(lengths) + 1) * 90                        # 90 slots per event: -1 rows for the short ones
    perm, node_map = sr.topk(torch.randn(N, generator=g0), sr.ptr_of(lengths), out_ptr, int(out_ptr[-1]))
    M = perm.numel()
    x, s, g = torch.randn(N, F, generator=g0), torch.randn(N, generator=g0), torch.randn(M, F, generator=g0)
    for gate in (s, None):
        sd = None if gate is None else gate.to(dev)
        fwd = pa.run_both(lambda: _native._select_rows(x.to(dev), sd, perm.to(dev)))
        bwd = pa.run_both(lambda: _native._select_rows_bwd(g.to(dev), x.to(dev), sd, node_map.to(dev)))
        want = sr.select_rows(x, gate, perm)
        want_gx, _fp32_gs, _ = sr.select_rows_bwd(g, x, gate, node_map)
        ref_gx, ref_gs, abs_sum = sr.select_rows_bwd(g.double(), x.double(), None if gate is None else gate.double(), node_map)
        for pattern in pa.PATTERNS:
            assert _same_bits(fwd[pattern][0], want), (F, pattern)
            assert _same_bits(bwd[pattern][0], want_gx), (F, pattern)
        assert torch.equal(bwd["ones"][1], bwd["zeros_huge"][1])
        _hold(f"F={F} gate={gate is not None} gs", bwd["ones"][1], ref_gs, sr.gamma(F) * abs_sum)
        unpicked = node_map < 0
        assert bool((bwd["ones"][0][unpicked] == 0).all()) and bool((bwd["ones"][1][unpicked] == 0).all())
        assert bool((fwd["ones"][0][perm < 0] == 0).all()) and int((perm < 0).sum()) > 0 and int(unpicked.sum()) > 0
        only_gx = _native._select_rows_bwd(g.to(dev), None, sd, node_map.to(dev), True, False)
        only_gs = _native._select_rows_bwd(g.to(dev), x.to(dev), sd, node_map.to(dev), False, True)
        assert only_gx[1] is None and only_gs[0] is None
        assert _same_bits(only_gx[0], want_gx) and torch.equal(only_gs[1].cpu(), bwd["ones"][1])


# ---- 5. the layers --------------------------------------------------------------------------------------------------------------
def _layer_inputs(F=6, seed=0, k=4):
    g = torch.Generator().manual_seed(90 + seed)
    lengths = sr.LAYER_LENGTHS
    N = sum(lengths)
    x = torch.randn(N, F, generator=g)
    ptr = sr.ptr_of(lengths).tolist()
    cols = []
    for b, n in enumerate(lengths):
        if n:
            cols.append(torch.randint(0, n, (2, 3 * n), generator=g) + ptr[b])
    ei = torch.cat(cols, 1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    nbr = torch.full((N, k), -1, dtype=torch.int32)
    for b, n in enumerate(lengths):
        if n:
            nbr[ptr[b]:ptr[b + 1]] = (torch.randint(0, n, (n, k), generator=g) + ptr[b]).to(torch.int32)
    nbr[torch.rand(N, k, generator=g) < 0.2] = -1
    return lengths, x, ei, nbr


def _tolerance(formula, *operands):
    """4 x the largest error of `formula` on fp32 CPU operands against the same formula in float64."""
    want = formula(*[t.double() for t in operands])
    return want, 4 * float((formula(*operands).double() - want).abs().max())


def _check_pooling(dev, layer, score_formula, score_operands, x, graph_in, lengths, ratio, multiplier, table=None):
    from deepmetv2_amd import NeighborTable
    from deepmetv2_amd.graph import batch_info
    batch = _register(lengths, dev)
    xg = x.to(dev).requires_grad_()
    g_in = NeighborTable(table.to(dev), sr.ptr_of(lengths).to(dev), dense=False, max_nodes=max(lengths)) if table is not None \
        else graph_in.to(dev)
    out, g2, attr2, batch2, perm, kept = layer(xg, g_in, None, batch)
    s = layer.scores(xg, g_in, batch)
    want_perm, want_map, out_ptr = sr.topk_ratio(s.detach().cpu(), lengths, ratio)
    assert torch.equal(perm.cpu(), want_perm)                     # the ranking of the layer's own scores, exactly
    score64, tol = _tolerance(score_formula, *score_operands)
    _hold("scores", s, score64, tol)

    def pooled(*ops):
        return sr.up_pool(ops[0], score_formula(*ops), want_perm, multiplier)[0]
    want_out, tol_out = _tolerance(pooled, *score_operands)
    _hold("x[perm] * score[perm]", out, want_out, tol_out)
    _hold("score[perm]", kept, score64[want_perm], tol)
    assert torch.equal(batch2.cpu(), sr.batch_of(lengths)[want_perm]) and attr2 is None
    info = batch_info(batch2, batch2.numel(), batch2.device)
    m = sr.slots_of(lengths, ratio)
    assert torch.equal(info.ptr.cpu(), out_ptr) and (info.num_events, info.max_nodes, info.min_nodes) == (len(lengths), max(m), min(m))
    if table is not None:
        want_nbr, want_cnt = sr.filter_table(table, None, want_perm, want_map)
        assert isinstance(g2, NeighborTable) and torch.equal(g2.nbr.cpu(), want_nbr) and torch.equal(g2.cnt.cpu(), want_cnt)
        assert torch.equal(g2.ptr.cpu(), out_ptr) and g2.max_nodes == max(m)
    else:
        assert torch.equal(g2.cpu(), sr.filter_edges(graph_in, want_map)[0])
    out.backward(torch.ones_like(out))
    grads = [xg.grad] + [p.grad for p in layer.parameters()]
    assert all(t is not None and bool(torch.isfinite(t).all()) and float(t.abs().sum()) > 0 for t in grads)
    return perm


@pytest.mark.parametrize("ratio,mult,act", [(0.5, 1.0, "tanh"), (0.3, 2.0, "sigmoid"), (5, 1.0, "tanh")])
@pytest.mark.parametrize("as_table", [False, True])
def test_topk_pooling_against_float64(dev, ratio, mult, act, as_table):
    from deepmetv2_amd import TopKPooling
    lengths, x, ei, nbr = _layer_inputs()
    torch.manual_seed(3)
    layer = TopKPooling(6, ratio, multiplier=mult, nonlinearity=act).to(dev)
    w = layer.select.weight.detach().cpu()
    _check_pooling(dev, layer, lambda xx, ww: sr.up_topk_score(xx, ww, getattr(torch, act)), (x, w), x, ei, lengths, ratio,
                   mult, nbr if as_table else None)


@pytest.mark.parametrize("as_table", [False, True])
def test_sag_pooling_against_float64(dev, as_table):
    from deepmetv2_amd import SAGPooling
    lengths, x, ei, nbr = _layer_inputs(seed=1)
    torch.manual_seed(4)
    layer = SAGPooling(6, 0.5).to(dev)
    names = list(layer.gnn.state_dict())
    params = [v.detach().cpu() for v in layer.gnn.state_dict().values()]
    edges = sr.table_edges(nbr) if as_table else ei

    def formula(xx, *ps):
        return torch.tanh(sr.up_graph_conv(xx, edges, dict(zip(names, ps))).view(-1))
    _check_pooling(dev, layer, formula, (x, *params), x, ei, lengths, 0.5, 1.0, nbr if as_table else None)


def test_topk_pooling_min_score_and_half_precision(dev):
    from deepmetv2_amd import TopKPooling
    lengths, x, ei, _nbr = _layer_inputs(seed=2)
    batch = _register(lengths, dev)
    torch.manual_seed(5)
    layer = TopKPooling(6, min_score=0.02).to(dev)
    out, ei2, _a, batch2, perm, kept = layer(x.to(dev), ei.to(dev), None, batch)
    s = layer.scores(x.to(dev), ei.to(dev), batch).cpu()
    want = sr.min_score_perm(s, sr.batch_of(lengths), len(lengths), 0.02)
    assert torch.equal(perm.cpu(), want) and torch.equal(batch2.cpu(), sr.batch_of(lengths)[want])
    w = layer.select.weight.detach().cpu()
    score64, tol = _tolerance(lambda xx, ww: sr.up_topk_score(xx, ww, None, sr.batch_of(lengths), len(lengths), 0.02), x, w)
    _hold("softmax scores", s, score64, tol)
    half = TopKPooling(6, 0.5).to(dev)
    for dt in (torch.bfloat16, torch.float16):
        xo, _e, _a, _b, p, sc = half(x.to(dev).to(dt), ei.to(dev), None, batch)
        assert xo.dtype == dt and sc.dtype == dt
        full = half.scores(x.to(dev).to(dt), ei.to(dev), batch)
        assert full.dtype == torch.float32 and torch.equal(p.cpu(), sr.topk_ratio(full.cpu(), lengths, 0.5)[0])
        want_x = sr.select_rows(x.to(dt).float(), full.cpu(), p.cpu()).to(dt)
        assert torch.equal(xo.cpu(), want_x)


def test_knn_graph_on_the_pooled_registered_batch_needs_no_sync(dev):
    from deepmetv2_amd import NeighborTable, TopKPooling, knn_graph, knn_table, raise_deferred_errors
    lengths = [40, 64, 33]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(sum(lengths), 5, generator=g).to(dev)
    batch = _register(lengths, dev)
    table = knn_table(x[:, :2].contiguous(), 8, batch)
    layer = TopKPooling(5, 16).to(dev)                  # an int ratio <= the registered min_nodes: M is known on the host
    warm = layer(x, table, None, batch)                 # warm-up: library load, allocator
    knn_graph(warm[0][:, :2].contiguous(), 8, warm[3], loop=True)
    with _NoSync():
        out, t2, _a, batch2, perm, _s = layer(x, table, None, batch)
        ei = knn_graph(out[:, :2].contiguous(), 8, batch2, loop=True)
    assert isinstance(t2, NeighborTable) and ei.shape == (2, 8 * perm.numel()) and perm.numel() == 3 * 16
    raise_deferred_errors()
    assert int(ei.min()) >= 0 and bool((batch2[ei[0]] == batch2[ei[1]]).all())


def test_no_sync_with_equal_registered_events_on_a_rounding_edge(dev):
    """50 * fp32(0.3) is above 15 in fp32 (fp32(0.3) > 0.3), so m = 16 where float64 gives 15: the host's M = B * 16 and the
    device's out_ptr must agree, or the kernel would cut slot ranges silently.  topk, and the layer over a table."""
    from deepmetv2_amd import NeighborTable, TopKPooling, topk
    B, n, k = 4, 50, 6
    lengths = [n] * B
    assert sr.m_of(n, 0.3) == 16
    g = torch.Generator().manual_seed(8)
    s, x = torch.randn(B * n, generator=g), torch.randn(B * n, 4, generator=g)
    nbr = (torch.randint(0, n, (B * n, k), generator=g) + (torch.arange(B * n) // n * n).view(-1, 1)).to(torch.int32)
    batch = _register(lengths, dev)
    table = NeighborTable(nbr.to(dev), sr.ptr_of(lengths).to(dev), dense=True, max_nodes=n)
    layer = TopKPooling(4, 0.3).to(dev)
    sd, xd = s.to(dev), x.to(dev)
    topk(sd, 0.3, batch, return_map=True), layer(xd, table, None, batch)          # warm-up
    with _NoSync():
        perm, node_map = topk(sd, 0.3, batch, return_map=True)
        out, t2, _a, batch2, lperm, _kept = layer(xd, table, None, batch)
    want_perm, want_map, out_ptr = sr.topk_ratio(s, lengths, 0.3)
    assert perm.shape == (B * 16,) and torch.equal(perm.cpu(), want_perm) and torch.equal(node_map.cpu(), want_map)
    assert int(perm.min()) >= 0
    lwant, lmap, _ = sr.topk_ratio(layer.scores(xd, table, batch).detach().cpu(), lengths, 0.3)
    assert lperm.shape == (B * 16,) and torch.equal(lperm.cpu(), lwant) and out.shape == (B * 16, 4)
    want_nbr, want_cnt = sr.filter_table(nbr, None, lwant, lmap)
    assert torch.equal(t2.nbr.cpu(), want_nbr) and torch.equal(t2.cnt.cpu(), want_cnt) and torch.equal(t2.ptr.cpu(), out_ptr)
    assert torch.equal(batch2.cpu(), sr.batch_of(lengths)[lwant]) and t2.max_nodes == 16


# ---- 6. global_sort_pool ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64, 400])
def test_global_sort_pool_equals_its_restatement(dev, k):
    from deepmetv2_amd import SortAggregation, global_sort_pool
    lengths = sr.LAYER_LENGTHS
    g = torch.Generator().manual_seed(11)
    x = torch.randn(sum(lengths), 5, generator=g)
    x[:, -1] = torch.randint(-3, 4, (x.shape[0],), generator=g).float()      # ties in the ranked channel
    batch = _register(lengths, dev)
    xg = x.to(dev).requires_grad_()
    global_sort_pool(xg, batch, k)                      # warm-up
    with _NoSync():
        got = global_sort_pool(xg, batch, k)
    want = sr.up_sort_pool(x, lengths, k)
    assert got.shape == want.shape and _same_bits(got.detach(), want)
    assert _same_bits(SortAggregation(k)(xg, batch).detach(), want)
    res = pa.run_both(lambda: global_sort_pool(x.to(dev), batch, k))
    assert _same_bits(res["ones"][0], want) and _same_bits(res["zeros_huge"][0], want)
    go = torch.randn(want.shape, generator=g)
    got.backward(go.to(dev))
    ptr = sr.ptr_of(lengths).tolist()
    ref = torch.zeros_like(x)
    for b, n in enumerate(lengths):
        order = sr.rank_event(x[ptr[b]:ptr[b + 1], -1].numpy())[:k]
        for slot, i in enumerate(order):
            ref[ptr[b] + i] = go[b].view(k, -1)[slot]
    assert _same_bits(xg.grad, ref)

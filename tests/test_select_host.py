"""deepmetv2_amd/select.py without a GPU: the key emulation against the ranking's definition, the select_rows gradients
against float64 autograd, the layers over tests/select_reference.FakeKernels against their float64 restatements, the m_b
rules, which paths form M without reading the device, state_dict keys, the refusals, the C entries' argument checks and
the export names.

The key-emulation tests (test_key_*) compare two functions of tests/select_reference.py with each other -- they check the
fake's ranking, run no code of the package and so also pass where the package has no select module; every other test here
needs it."""
import math
import os

import numpy as np
import pytest
import torch

import select_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    """The tests of this file seed and draw from torch's global generators; what later tests find there stays as it was."""
    with torch.random.fork_rng(devices=[0] if torch.cuda.is_available() else []):
        yield


@pytest.fixture
def fake(monkeypatch):
    return sr.FakeKernels().install(monkeypatch)


def _registered(lengths):
    from deepmetv2_amd import register_batch
    batch = sr.batch_of(lengths)
    register_batch(batch, sr.ptr_of(lengths), len(lengths), max_nodes=max(lengths), min_nodes=min(lengths))
    return batch


class _NoRead:
    """Makes .item() / .tolist() of any tensor raise for the duration of a block."""

    def __enter__(self):
        def boom(*_a, **_k):
            raise AssertionError("the device was read (.item() / .tolist())")
        self.saved = (torch.Tensor.item, torch.Tensor.tolist)
        torch.Tensor.item = torch.Tensor.tolist = boom

    def __exit__(self, *exc):
        torch.Tensor.item, torch.Tensor.tolist = self.saved


# ---- the key ------------------------------------------------------------------------------------------------------------------
def test_key_orders_the_special_values_as_the_definition_does():
    nan_variants = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    vals = np.concatenate([sr.SPECIALS, nan_variants, np.array([1e-45, -1e-45, 3.4e38, -3.4e38, 1.0, 1.0], dtype=np.float32)])
    assert sr.rank_event_by_key(vals) == sr.rank_event(vals)
    order = sr.rank_event(vals)
    n_nan = int(np.isnan(vals).sum())
    assert all(math.isnan(vals[i]) for i in order[:n_nan]) and order[:n_nan] == sorted(order[:n_nan])   # NaN first, by index
    assert vals[order[n_nan]] == np.inf and vals[order[-1]] == -np.inf
    zeros = [i for i in order if vals[i] == 0.0]
    assert zeros == sorted(zeros) and len(zeros) == 4                       # -0.0 ties with +0.0: index order
    assert sr.select_key(np.float32(-0.0), 5) == sr.select_key(np.float32(0.0), 5)
    assert sr.select_key(nan_variants[1], 0) >> 32 == 0xFFFFFFFF            # a negative NaN does not land at the bottom
    assert sr.select_key(np.float32(-np.inf), 2 ** 31 - 2) > 0


@pytest.mark.parametrize("kind", sr.KINDS)
def test_key_ranking_equals_the_definition_on_every_score_kind(kind):
    lengths = [0, 1, 2, 63, 64, 65, 300, 0]
    s, ptr = sr.scores(kind, lengths).numpy(), sr.ptr_of(lengths).tolist()
    for b in range(len(lengths)):
        ev = s[ptr[b]:ptr[b + 1]]
        assert sr.rank_event_by_key(ev) == sr.rank_event(ev)
    if kind == "special" and len(s):
        want = torch.sort(torch.from_numpy(s[ptr[6]:ptr[7]]), descending=True, stable=True).values.numpy()
        got = s[ptr[6]:ptr[7]][sr.rank_event(s[ptr[6]:ptr[7]])]
        assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(want[~np.isnan(want)], got[~np.isnan(got)])


# ---- m_b ----------------------------------------------------------------------------------------------------------------------
def test_m_rules_on_the_host_and_in_torch_agree():
    from deepmetv2_amd import select
    ns = [0, 1, 2, 3, 7, 10, 64, 100, 4500, 16384, 16777217]
    for ratio in (1.0, 0.5, 1e-4, 0.3, 0.7, 1 / 3, 1, 30):
        dev = select._m_device(torch.tensor(ns), ratio).tolist()
        assert dev == [select._m_host(n, ratio) for n in ns] == [sr.m_of(n, ratio) for n in ns], ratio
    assert sr.m_of(50, 0.3) == 16 and math.ceil(50 * 0.3) == 15    # fp32(0.3) > 0.3: the fp32 product is above 15
    assert sr.m_of(5, 1e-4) == 1 and sr.m_of(0, 1e-4) == 0 and sr.m_of(4500, 1e-4) == 1     # tiny ratios keep one node
    assert sr.m_of(7, 30) == 7 and sr.m_of(31, 30) == 30                                    # events shorter than ratio


@pytest.mark.parametrize("ratio", [0, -1, 0.0, 1.5, -0.5, True, False, "0.5", None, float("nan")])
def test_bad_ratio_is_refused(fake, ratio):
    from deepmetv2_amd import TopKPooling, SAGPooling, topk
    with pytest.raises(ValueError, match="ratio"):
        topk(torch.randn(4), ratio, _registered([4]))
    with pytest.raises(ValueError, match="ratio"):
        TopKPooling(4, ratio)
    with pytest.raises(ValueError, match="ratio"):
        SAGPooling(4, ratio, GNN=_TorchGraphConv)


@pytest.mark.parametrize("ratio", sr.RATIOS)
def test_topk_over_the_fake_equals_the_reference(fake, ratio):
    from deepmetv2_amd import topk
    lengths = [0, 1, 2, 40, 64, 65, 0, 29, 30, 31]
    for kind in sr.KINDS:
        s = sr.scores(kind, lengths)
        perm, node_map = topk(s, ratio, _registered(lengths), return_map=True)
        want_perm, want_map, _ = sr.topk_ratio(s, lengths, ratio)
        assert torch.equal(perm, want_perm) and torch.equal(node_map, want_map), (kind, ratio)
        assert perm.dtype == torch.int64 and node_map.dtype == torch.int32 and int((perm < 0).sum()) == 0
        assert torch.equal(topk(s, ratio, ptr=sr.ptr_of(lengths)), want_perm)


def test_m_is_formed_without_reading_the_device(fake):
    from deepmetv2_amd import topk
    s = sr.scores("gauss", [50] * 6)
    equal, ragged = _registered([50] * 6), _registered([40, 31, 64, 30, 50, 85])
    with _NoRead():
        p1 = topk(s, 0.5, equal)                    # equal event sizes, float ratio
        p2 = topk(s, 7, equal)                      # equal event sizes, int ratio
        p3 = topk(s, 30, ragged)                    # ragged, registered min_nodes = 30 >= ratio
    assert p1.numel() == 6 * 25 and p2.numel() == 6 * 7 and p3.numel() == 6 * 30
    assert torch.equal(p3, sr.topk_ratio(s, [40, 31, 64, 30, 50, 85], 30)[0])
    with _NoRead(), pytest.raises(AssertionError, match="device was read"):
        topk(s, 31, ragged)                         # min_nodes < ratio: M costs the one read
    with _NoRead(), pytest.raises(AssertionError, match="device was read"):
        topk(s, 0.5, ragged)


def test_min_score_rule(fake):
    from deepmetv2_amd import topk
    lengths = [5, 1, 8]
    batch = _registered(lengths)
    s = torch.tensor([.1, .9, .5, .9, .2, .3, .1, .2, .3, .4, .5, .6, .7, .05])
    import deepmetv2_amd.select as sel
    # scatter_max is a kernel of its own: stand in for it with torch
    def fake_max(src, index, dim=0, out=None, dim_size=None):
        return (torch.full((dim_size, 1), -float("inf")).scatter_reduce(0, index.view(-1, 1), src, "amax"), None)
    orig = sel.scatter_max
    sel.scatter_max = fake_max
    try:
        perm, node_map = topk(s, None, batch, min_score=0.45, return_map=True)
        high = topk(s, None, batch, min_score=5.0)          # above every score: max_b - tol keeps each event's maximum
    finally:
        sel.scatter_max = orig
    assert torch.equal(perm, sr.min_score_perm(s, batch, 3, 0.45)) and perm.tolist() == [1, 2, 3, 5, 10, 11, 12]
    assert node_map.tolist() == [-1, 0, 1, 2, -1, 3] + [-1] * 4 + [4, 5, 6, -1]      # a lone node is its event's maximum
    assert torch.equal(high, sr.min_score_perm(s, batch, 3, 5.0)) and high.tolist() == [1, 3, 5, 12]
    assert "topk" not in fake.calls                          # that path is not the kernel


# ---- select_rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 64, 65])
def test_select_rows_gradients_against_float64_autograd(fake, F):
    from deepmetv2_amd.select import select_rows
    g0 = torch.Generator().manual_seed(F)
    N = 40
    perm = torch.tensor([7, 3, -1, 39, 0, 12, -1])
    node_map = torch.full((N,), -1, dtype=torch.int32)
    node_map[perm[perm >= 0]] = torch.arange(perm.numel(), dtype=torch.int32)[perm >= 0]
    x = torch.randn(N, F, generator=g0, requires_grad=True)
    s = torch.randn(N, generator=g0, requires_grad=True)
    go = torch.randn(perm.numel(), F, generator=g0)
    for with_s in (True, False):
        out = select_rows(x, s if with_s else None, perm, node_map)
        gx, gs = torch.autograd.grad(out, (x, s) if with_s else (x,), go) + (() if with_s else (None,))
        xd, sd = x.detach().double().requires_grad_(), s.detach().double().requires_grad_()
        ok = (perm >= 0).view(-1, 1)
        ref = torch.where(ok, xd[perm.clamp(min=0)] * (sd[perm.clamp(min=0)].view(-1, 1) if with_s else 1.0), torch.zeros(1, dtype=torch.float64))
        rgx, rgs = torch.autograd.grad(ref, (xd, sd), go.double(), allow_unused=True)
        assert torch.equal(out, ref.float())                                    # one multiply: the rounded float64 product
        assert torch.equal(gx, rgx.float())
        picked = node_map >= 0
        assert bool((gx[~picked] == 0).all()) and bool((out[perm < 0] == 0).all())
        if with_s:
            bound = sr.gamma(F) * (go.double()[node_map.clamp(min=0).long()] * x.detach().double()).abs().sum(1) * picked
            assert bool(((gs.double() - rgs).abs() <= bound).all()) and bool((gs[~picked] == 0).all())
    assert fake.calls["select_rows_bwd"] == 2


def test_only_the_needed_gradients_are_formed(fake, monkeypatch):
    import deepmetv2_amd._native as nat
    from deepmetv2_amd.select import select_rows
    asked = []
    inner = nat._select_rows_bwd
    monkeypatch.setattr(nat, "_select_rows_bwd", lambda g, x, s, nm, need_gx=True, need_gs=True:
                        (asked.append((need_gx, need_gs, x is None)), inner(g, x, s, nm, need_gx, need_gs))[1])
    perm, node_map = torch.tensor([1, 0]), torch.tensor([1, 0, -1], dtype=torch.int32)
    x, s = torch.randn(3, 4), torch.randn(3)
    select_rows(x.clone().requires_grad_(), s, perm, node_map).sum().backward()
    select_rows(x, s.clone().requires_grad_(), perm, node_map).sum().backward()
    select_rows(x.clone().requires_grad_(), None, perm, node_map).sum().backward()
    assert asked == [(True, False, True), (False, True, False), (True, False, True)]      # x is kept for gs alone


# ---- the layers ----------------------------------------------------------------------------------------------------------------
class _TorchGraphConv(torch.nn.Module):
    """GraphConv's formula from torch operators over an int64 [2, E] edge index (the package's own runs a kernel)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin_rel = torch.nn.Linear(in_channels, out_channels)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x, edge_index):
        agg = torch.zeros_like(x).index_add(0, edge_index[1], x[edge_index[0]])
        return self.lin_rel(agg) + self.lin_root(x)


def _graph(lengths, seed=3, deg=4):
    """Random edges inside the events, duplicates and self loops included, in no order."""
    g = torch.Generator().manual_seed(seed)
    ptr = sr.ptr_of(lengths).tolist()
    rows = []
    for b, n in enumerate(lengths):
        if n:
            e = torch.randint(0, n, (2, deg * n), generator=g) + ptr[b]
            rows.append(e)
    ei = torch.cat(rows, 1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)]


LAYER_LENGTHS = [0, 1, 2, 17, 33, 0, 40]


def _check_layer(layer, x, ei, lengths, score64, ratio, multiplier, edge_attr=None):
    batch = _registered(lengths)
    out, ei2, attr2, batch2, perm, kept = layer(x, ei, edge_attr, batch)
    s = layer.scores(x, ei, batch)
    want_perm, want_map, out_ptr = sr.topk_ratio(s.detach(), lengths, ratio)
    assert torch.equal(perm, want_perm)
    assert float((s.detach().double() - score64).abs().max()) < 1e-5
    want_out, want_kept = sr.up_pool(x.detach().double(), score64, perm, multiplier)
    assert float((out.detach().double() - want_out).abs().max()) < 1e-5 and float((kept.detach().double() - want_kept).abs().max()) < 1e-5
    want_ei, want_keep, _ = sr.filter_edges(ei, want_map)
    assert torch.equal(ei2, want_ei) and torch.equal(batch2, batch[perm])
    if edge_attr is not None:
        assert torch.equal(attr2, edge_attr[want_keep])
    else:
        assert attr2 is None
    from deepmetv2_amd.graph import batch_info
    info = batch_info(batch2, batch2.numel(), batch2.device)
    m = sr.slots_of(lengths, ratio)
    assert torch.equal(info.ptr, out_ptr) and (info.num_events, info.max_nodes, info.min_nodes) == (len(lengths), max(m), min(m))
    return out, perm


@pytest.mark.parametrize("ratio,mult,act", [(0.5, 1.0, "tanh"), (0.3, 2.0, "sigmoid"), (5, 1.0, "tanh")])
def test_topk_pooling_over_the_fakes_against_float64(fake, ratio, mult, act):
    from deepmetv2_amd import TopKPooling
    torch.manual_seed(1)
    layer = TopKPooling(6, ratio, multiplier=mult, nonlinearity=act)
    x = torch.randn(sum(LAYER_LENGTHS), 6, requires_grad=True)
    ei = _graph(LAYER_LENGTHS)
    attr = torch.randn(ei.shape[1], 2)
    w = layer.select.weight.detach().double()
    score64 = sr.up_topk_score(x.detach().double(), w, getattr(torch, act))
    out, perm = _check_layer(layer, x, ei, LAYER_LENGTHS, score64, ratio, mult, attr)
    out.sum().backward()
    assert x.grad is not None and layer.select.weight.grad is not None
    picked = torch.zeros(x.shape[0], dtype=torch.bool)
    picked[perm] = True
    assert bool((x.grad[picked].abs().sum(1) > 0).all())


def test_sag_pooling_over_the_fakes_against_float64(fake):
    from deepmetv2_amd import SAGPooling
    torch.manual_seed(2)
    layer = SAGPooling(6, 0.5, GNN=_TorchGraphConv)
    x = torch.randn(sum(LAYER_LENGTHS), 6, requires_grad=True)
    ei = _graph(LAYER_LENGTHS)
    p = {k: v.detach().double() for k, v in layer.gnn.state_dict().items()}
    score64 = torch.tanh(sr.up_graph_conv(x.detach().double(), ei, p).view(-1))
    out, _perm = _check_layer(layer, x, ei, LAYER_LENGTHS, score64, 0.5, 1.0)
    out.sum().backward()
    assert x.grad is not None and all(q.grad is not None for q in layer.gnn.parameters())


def test_table_in_gives_table_out_without_reading_the_device(fake):
    from deepmetv2_amd import NeighborTable, TopKPooling
    lengths = [20] * 4
    N, k = sum(lengths), 5
    g = torch.Generator().manual_seed(4)
    nbr = (torch.randint(0, 20, (N, k), generator=g) + (torch.arange(N) // 20 * 20).view(-1, 1)).to(torch.int32)
    nbr[torch.rand(N, k, generator=g) < 0.2] = -1
    table = NeighborTable(nbr, sr.ptr_of(lengths), dense=False, max_nodes=20)
    layer = TopKPooling(3, 0.5)
    x = torch.randn(N, 3)
    batch = _registered(lengths)
    with _NoRead():
        out, t2, attr2, batch2, perm, _kept = layer(x, table, None, batch)
    assert isinstance(t2, NeighborTable) and attr2 is None and not t2.dense and t2.max_nodes == 10 and t2.k == k
    want_perm, want_map, out_ptr = sr.topk_ratio(layer.scores(x, table, batch).detach(), lengths, 0.5)
    want_nbr, want_cnt = sr.filter_table(nbr, None, want_perm, want_map)
    assert torch.equal(t2.nbr, want_nbr) and torch.equal(t2.cnt, want_cnt) and torch.equal(t2.ptr, out_ptr)
    assert fake.calls.get("filter_edges") is None


def test_global_sort_pool_over_the_fakes(fake):
    from deepmetv2_amd import SortAggregation, global_sort_pool
    lengths = [0, 1, 4, 5, 6, 9]
    x = torch.randn(sum(lengths), 3, requires_grad=True)
    x.data[7:10, -1] = 0.5                                  # ties in the ranked channel
    batch = _registered(lengths)
    for k in (1, 5, 12):
        with _NoRead():
            got = global_sort_pool(x, batch, k)
        assert got.shape == (len(lengths), 3 * k) and torch.equal(got.detach(), sr.up_sort_pool(x.detach(), lengths, k))
    assert torch.equal(SortAggregation(5)(x, batch).detach(), sr.up_sort_pool(x.detach(), lengths, 5))
    got.sum().backward()
    assert torch.equal(x.grad, torch.ones_like(x))          # k = 12 >= every event: every row is gathered once


# ---- state_dict, refusals, exports ----------------------------------------------------------------------------------------------
def test_state_dict_keys_and_the_legacy_weight():
    from deepmetv2_amd import SAGPooling, TopKPooling
    layer = TopKPooling(8)
    assert list(layer.state_dict()) == ["select.weight"] and layer.select.weight.shape == (1, 8)
    w = torch.randn(1, 8)
    layer.load_state_dict({"weight": w})
    assert torch.equal(layer.select.weight, w)
    layer.load_state_dict({"select.weight": w * 2})
    assert torch.equal(layer.select.weight, w * 2)
    nested = torch.nn.Sequential(TopKPooling(8))
    nested.load_state_dict({"0.weight": w})
    assert torch.equal(nested[0].select.weight, w)
    assert sorted(SAGPooling(8).state_dict()) == ["gnn.lin_rel.bias", "gnn.lin_rel.weight", "gnn.lin_root.weight"]


def test_refusals(fake):
    from deepmetv2_amd import BipartiteTable, NeighborTable, SAGPooling, TopKPooling, filter_table
    nbr = torch.zeros(4, 2, dtype=torch.int32)
    ptr = torch.tensor([0, 4])
    bip = BipartiteTable(nbr, ptr, ptr, 4)
    table = NeighborTable(nbr, ptr, dense=True, max_nodes=4)
    x = torch.randn(4, 3)
    for layer in (TopKPooling(3), SAGPooling(3, GNN=_TorchGraphConv)):
        with pytest.raises(ValueError, match="BipartiteTable"):
            layer(x, bip)
        with pytest.raises(ValueError, match="edge_attr"):
            layer(x, table, torch.randn(8, 1))
        with pytest.raises(ValueError, match="edge_index"):
            layer(x, torch.zeros(3, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="BipartiteTable"):
        filter_table(bip, torch.zeros(1, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), ptr)
    with pytest.raises(ValueError, match="k must be"):
        from deepmetv2_amd import SortAggregation
        SortAggregation(0)


def test_exports():
    import deepmetv2_amd as d
    for name in ("TopKPooling", "SAGPooling", "SortAggregation", "global_sort_pool", "topk", "filter_adj", "filter_table"):
        assert name in d.__all__ and hasattr(d, name) and name in d.__doc__, name


# ---- the C entries' argument checks --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdmet_hip.so is not built")
    return _lib.load()


def test_c_entries_check_their_arguments_before_any_hip_call(lib):
    def bad(rc, *words):
        msg = lib.dmet_last_error()
        assert rc == -22 and all(w in msg for w in words), (rc, msg)

    P = 1 << 20         # a non-NULL address nothing dereferences: every call below is refused or empty before a launch
    bad(lib.dmet_topk_f32(P, P, 1, -1, P, 1, P, P, P, 1 << 30, None), b"dmet_topk_f32", b"N=-1")
    bad(lib.dmet_topk_f32(P, P, -1, 4, P, 1, P, P, P, 1 << 30, None), b"B=-1")
    bad(lib.dmet_topk_f32(P, P, 1, 4, P, -2, P, P, P, 1 << 30, None), b"M=-2")
    bad(lib.dmet_topk_f32(P, P, 1, 4, P, 1, P, P, P, 8, None), b"ws_bytes=8")
    bad(lib.dmet_topk_f32(None, P, 1, 4, P, 1, P, P, P, 1 << 30, None), b"score is NULL")
    bad(lib.dmet_topk_f32(P, None, 1, 4, P, 1, P, P, P, 1 << 30, None), b"ptr is NULL")
    bad(lib.dmet_topk_f32(P, P, 1, 4, None, 1, P, P, P, 1 << 30, None), b"out_ptr is NULL")
    bad(lib.dmet_topk_f32(P, P, 1, 4, P, 1, None, P, P, 1 << 30, None), b"perm is NULL")
    bad(lib.dmet_topk_f32(P, P, 1, 4, P, 1, P, None, P, 1 << 30, None), b"node_map is NULL")
    bad(lib.dmet_topk_f32(P, P, 1, 4, P, 1, P, P, None, 1 << 30, None), b"ws is NULL")
    assert lib.dmet_topk_f32(None, None, 0, 4, None, 1, None, None, None, 0, None) == 0
    assert lib.dmet_topk_f32(None, None, 3, 0, None, 0, None, None, None, 0, None) == 0
    assert lib.dmet_topk_workspace_bytes(1000) == 16000 and lib.dmet_topk_workspace_bytes(0) == 0
    bad(lib.dmet_select_rows_f32(P, None, P, 4, 2, 0, P, None), b"dmet_select_rows_f32", b"F=0")
    bad(lib.dmet_select_rows_f32(None, None, P, 4, 2, 3, P, None), b"x is NULL")
    bad(lib.dmet_select_rows_f32(P, None, None, 4, 2, 3, P, None), b"perm is NULL")
    bad(lib.dmet_select_rows_f32(P, None, P, 4, 2, 3, None, None), b"out is NULL")
    assert lib.dmet_select_rows_f32(None, None, None, 4, 0, 3, None, None) == 0
    bad(lib.dmet_select_rows_bwd_f32(P, P, None, P, 4, 2, 0, P, P, None), b"dmet_select_rows_bwd_f32", b"F=0")
    bad(lib.dmet_select_rows_bwd_f32(None, P, None, P, 4, 2, 3, P, P, None), b"g is NULL")
    bad(lib.dmet_select_rows_bwd_f32(P, P, None, None, 4, 2, 3, P, P, None), b"node_map is NULL")
    bad(lib.dmet_select_rows_bwd_f32(P, None, None, P, 4, 2, 3, P, P, None), b"x is NULL")
    assert lib.dmet_select_rows_bwd_f32(None, None, None, None, 4, 2, 3, None, None, None) == 0     # nobody needs a gradient
    assert lib.dmet_select_rows_bwd_f32(None, None, None, None, 0, 2, 3, P, P, None) == 0
    bad(lib.dmet_filter_table(P, None, P, P, 4, 2, 0, P, P, None), b"dmet_filter_table", b"k=0")
    bad(lib.dmet_filter_table(P, None, P, P, 4, 2, 1025, P, P, None), b"k=1025")
    bad(lib.dmet_filter_table(None, None, P, P, 4, 2, 8, P, P, None), b"nbr is NULL")
    bad(lib.dmet_filter_table(P, None, None, P, 4, 2, 8, P, P, None), b"perm is NULL")
    bad(lib.dmet_filter_table(P, None, P, None, 4, 2, 8, P, P, None), b"node_map is NULL")
    bad(lib.dmet_filter_table(P, None, P, P, 4, 2, 8, None, P, None), b"out_nbr is NULL")
    bad(lib.dmet_filter_table(P, None, P, P, 4, 2, 8, P, None, None), b"out_cnt is NULL")
    assert lib.dmet_filter_table(None, None, None, None, 4, 0, 8, None, None, None) == 0
    ws = lib.dmet_filter_edges_workspace_bytes(5000)
    assert ws >= 6 * 8 + 5 * 4 and lib.dmet_filter_edges_workspace_bytes(0) == 0
    bad(lib.dmet_filter_edges_count(P, P, -1, P, 4, P, P, P, ws, None), b"dmet_filter_edges_count", b"E=-1")
    bad(lib.dmet_filter_edges_count(P, P, 5000, P, 4, P, P, P, 8, None), b"ws_bytes=8")
    bad(lib.dmet_filter_edges_count(None, P, 5000, P, 4, P, P, P, ws, None), b"row is NULL")
    bad(lib.dmet_filter_edges_count(P, P, 5000, P, 4, None, P, P, ws, None), b"total is NULL")
    bad(lib.dmet_filter_edges_count(P, P, 5000, P, 4, P, None, P, ws, None), b"nbad is NULL")
    assert lib.dmet_filter_edges_count(None, None, 0, None, 4, None, None, None, 0, None) == 0
    bad(lib.dmet_filter_edges_write(P, P, 5000, P, 4, P, ws, 5001, P, P, None), b"dmet_filter_edges_write", b"Eout=5001")
    bad(lib.dmet_filter_edges_write(P, P, 5000, P, 4, P, ws, 10, None, P, None), b"out_index is NULL")
    bad(lib.dmet_filter_edges_write(P, P, 5000, P, 4, P, ws, 10, P, None, None), b"kept is NULL")
    assert lib.dmet_filter_edges_write(None, None, 5000, None, 4, None, 0, 0, None, None, None) == 0

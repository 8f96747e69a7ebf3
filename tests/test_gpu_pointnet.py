"""PointNetConv on the GPU (csrc/pointnet.hip, deepmetv2_amd/pointnet.py) against the float64 reference of
tests/pointnet_reference.py over the same graph -- the table or list the GPU built.

Bar: the output within 1e-4 of its scale (max |reference|), every gradient within 1e-4 of its own tensor's scale: the
project's stated bar for the split-first-Linear construction (include/dmet.h, fp32 edge MLP).  Exact, not bars: zero rows
for targets without an entry, zero gradients for sources nobody lists, and the win codes.  Every case searches
pointnet_cases.TRIES deterministic seeds for inputs without fragile elements (tests/pointnet_reference.py) over the graph
the GPU built and fails, not skips, when none is clear; tests/test_pointnet_host.py shows on the CPU that the search
succeeds for every case.  Each test prints its ratios error / scale; measured on an MI355X the largest over all fp32
cases is 4.3e-7 (3.5e-3 under bf16 autocast, against 2e-2)."""
import pytest
import torch

import pointnet_cases as pc
import pointnet_reference as pr
import poisoned_alloc as pa

pytestmark = pytest.mark.gpu

BAR = 1e-4
BF16_BAR = 2e-2     # rule R6


def _to(inp, dev):
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    if inp["pos_dst"] is inp["pos_src"]:
        d["pos_dst"] = d["pos_src"]          # one node set stays one tensor
    return d


def _graph(case, d, loop=True, pad=False):
    """The case's graph on the device: (what PointNetConv takes as edge_index, the reference's entries)."""
    import deepmetv2_amd as dm
    c = pc.CASES[case]
    Ns, Nt = pc.sizes(case)
    kind = c["graph"][0]
    B = len(c["src"])
    if kind == "list":
        ei = d["edge_index"]
        return ei, pr.entries_from_list(ei[0].cpu(), ei[1].cpu(), Nt, c["self_loop"])
    if kind == "radius":
        table = dm.radius_xy_table(d["pos_src"], d["pos_dst"], c["graph"][1], d["batch_src"], d["batch_dst"],
                                   max_num_neighbors=c["graph"][2], batch_size=B, pad=pad)
        return table, pr.entries_from_table(table.nbr.cpu(), Ns, table.cnt.cpu(), False)
    if c["dst"] is None:
        # k other nodes either way: loop=True writes the node itself into its row as well (the layer skips it again)
        table = dm.knn_table(d["pos_src"], c["graph"][1] + (1 if loop else 0), d["batch_src"], loop=loop, num_events=B)
    else:
        table = dm.knn_xy_table(d["pos_src"], d["pos_dst"], c["graph"][1], d["batch_src"], d["batch_dst"], batch_size=B)
    return table, pr.entries_from_table(table.nbr.cpu(), Ns, None, c["self_loop"])


def _layer(case, d, **kw):
    import deepmetv2_amd as dm
    c = pc.CASES[case]
    A = torch.nn.ReLU if c["act"] == "relu" else torch.nn.ELU
    bias = d["b1"] is not None
    mods = [torch.nn.Linear(c["F"] + c["D"], c["H1"], bias=bias), A(), torch.nn.Linear(c["H1"], c["H2"], bias=bias)]
    if c["act2"]:
        mods.append(A())
    conv = dm.PointNetConv(torch.nn.Sequential(*mods), add_self_loops=c["self_loop"], **kw).to(d["W1"].device)
    with torch.no_grad():
        conv.local_nn[0].weight.copy_(d["W1"])
        conv.local_nn[2].weight.copy_(d["W2"])
        if bias:
            conv.local_nn[0].bias.copy_(d["b1"])
            conv.local_nn[2].bias.copy_(d["b2"])
    return conv


def _gout(case, dev):
    _Ns, Nt = pc.sizes(case)
    return torch.randn(Nt, pc.CASES[case]["H2"], generator=torch.Generator().manual_seed(5)).to(dev)


def _run(case, d, graph, conv=None, g=None):
    """Forward + backward through PointNetConv: (out, {name: gradient}); one set: 'pos' is the position's whole gradient."""
    c = pc.CASES[case]
    conv = _layer(case, d) if conv is None else conv
    conv.zero_grad()
    x = None if d["x"] is None else d["x"].detach().requires_grad_(True)       # shares storage: a view stays a view
    ps = d["pos_src"].detach().requires_grad_(True)
    one = c["dst"] is None
    pd = ps if one else d["pos_dst"].detach().requires_grad_(True)
    out = conv(x if one else (x, None), ps if one else (ps, pd), graph)
    out.backward(_gout(case, out.device) if g is None else g)
    grads = {"W1": conv.local_nn[0].weight.grad, "W2": conv.local_nn[2].weight.grad}
    if conv.local_nn[0].bias is not None:
        grads["b1"], grads["b2"] = conv.local_nn[0].bias.grad, conv.local_nn[2].bias.grad
    if x is not None:
        grads["x"] = x.grad
    if one:
        grads["pos"] = ps.grad
    else:
        grads["pos_src"], grads["pos_dst"] = ps.grad, pd.grad
    return out.detach(), {k: v.detach().clone() for k, v in grads.items()}


def _close(got, ref, what, bar=BAR):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    if scale == 0.0:
        assert err == 0.0, (what, err)
        return 0.0
    print(f"{what}: max err / scale {err / scale:.3e}")
    assert err <= bar * scale, (what, err / scale)
    return err / scale


def _check(case, d, ref, out, grads, bar=BAR):
    c = pc.CASES[case]
    _close(out, ref.out, f"{case} out", bar)
    empty = (ref.win == -1).all(1)
    assert bool((out.cpu()[empty] == 0).all()), case                      # R3, exactly
    rg = ref.backward(_gout(case, "cpu"))
    if c["dst"] is None:
        rg["pos"] = rg.pop("pos_src") + rg.pop("pos_dst")
    for name, got in grads.items():
        _close(got, rg[name], f"{case} g_{name}", bar)
    unlisted = ~ref.listed()
    for name in ("x", "pos_src"):
        if name in grads:
            assert bool((grads[name].cpu()[unlisted] == 0).all()), (case, name)   # a source nobody lists, exactly


def _found(case, dev, **kw):
    """The seed search over the graph the GPU builds: (device inputs, graph, reference)."""
    box = {}

    def entries_of(inp):
        d = _to(inp, dev)
        graph, entries = _graph(case, d, **kw)
        box["d"], box["graph"] = d, graph
        return entries
    _seed, _inp, _entries, ref = pc.find_seed(case, entries_of)
    return box["d"], box["graph"], ref


def _winners(case, d, graph):
    """(out, win) of pointnet_aggregate itself over the case's graph (a tensor edge index as its EdgeList)."""
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import edge_list_from_edge_index
    c = pc.CASES[case]
    Ns, Nt = pc.sizes(case)
    conv = _layer(case, d)
    if torch.is_tensor(graph):
        graph = edge_list_from_edge_index(graph, Nt, "source_to_target", num_src=None if c["dst"] is None else Ns)
    with torch.no_grad():
        return dm.pointnet_aggregate(d["x"], d["pos_src"], d["pos_dst"], graph, conv.local_nn[0], conv.local_nn[2], c["act"],
                                     c["act2"], c["self_loop"], return_winners=True)


# ---- 1. cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pc.CASES))
def test_cases(dev, case):
    d, graph, ref = _found(case, dev)
    out, grads = _run(case, d, graph)
    _check(case, d, ref, out, grads)
    raw, win = _winners(case, d, graph)
    assert torch.equal(raw, out)                                         # the module adds nothing to the operator
    assert torch.equal(win.cpu().long(), ref.win), case                  # the codes, exactly
    # two runs, the same bits
    out2, grads2 = _run(case, d, graph)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads), case
    c = pc.CASES[case]
    if case == "smallest":
        assert bool((win == -2).all())                                   # the added self entry alone
    if case == "set abstraction":
        assert int((graph.nbr[10:] >= 0).sum(1).max()) == 7              # event 2 has short rows
    if case == "empty events":
        assert bool((win[3:] == -1).all()) and bool((out[3:] == 0).all())
        assert bool((grads["x"][:5] != 0).any()) and bool((grads["x"][5:] == 0).all())     # event 2's sources: no target
    if case == "radius":
        assert graph.cnt is not None and c["graph"][2] == graph.k


def test_table_and_list_give_equal_bits(dev):
    for case in ("set abstraction", "one set", "limits"):
        d, table, _ref = _found(case, dev)
        out_t, grads_t = _run(case, d, table)
        edges = table.edge_list()
        c = pc.CASES[case]
        ei = torch.stack([edges.src.long(), edges.tgt.long()])
        out_l, grads_l = _run(case, d, ei)
        assert torch.equal(out_t, out_l), case
        for k in grads_t:
            assert torch.equal(grads_t[k], grads_l[k]), (case, k)
        assert c["self_loop"] == (case == "one set")


def test_one_set_with_and_without_written_self_loops(dev):
    case = "one set"
    d, with_loops, ref = _found(case, dev, loop=True)
    without, entries = _graph(case, d, loop=False)
    assert bool((with_loops.nbr[:, 0] == torch.arange(with_loops.num_nodes, device=dev)).all())    # written self loops
    ref2 = pc.reference(case, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}, entries)
    assert torch.equal(ref.out, ref2.out)                                # the same graph once the loops are rewritten
    out_a, grads_a = _run(case, d, with_loops)
    out_b, grads_b = _run(case, d, without)
    _check(case, d, ref, out_a, grads_a)
    assert torch.equal(out_a, out_b)
    for k in grads_a:
        _close(grads_b[k], grads_a[k].cpu(), f"one set, loop=False, g_{k}")


def test_counted_table_ignores_slots_beyond_cnt(dev):
    import deepmetv2_amd as dm
    case = "radius"
    d, table, ref = _found(case, dev)
    conv = _layer(case, d)
    slot = torch.arange(table.k, device=dev).view(1, -1)
    beyond = slot >= table.cnt.view(-1, 1)
    assert bool(beyond.any())
    with torch.no_grad():
        clean = conv((d["x"], None), (d["pos_src"], d["pos_dst"]), table)
        outs = []
        for poison in (0, 3, -1, 2 ** 30):
            nbr = torch.where(beyond, torch.full_like(table.nbr, poison), table.nbr)
            t2 = dm.BipartiteTable(nbr, table.ptr_x, table.ptr_y, table.num_candidates, cnt=table.cnt)
            outs.append(conv((d["x"], None), (d["pos_src"], d["pos_dst"]), t2))
    _close(clean, ref.out, "radius, no grad (table form)")
    assert all(torch.equal(o, clean) for o in outs)
    out, grads = _run(case, d, table)                                    # with gradients: through the edge list
    assert torch.equal(out, clean)


def test_unaligned_views(dev):
    case = "set abstraction"
    d, graph, ref = _found(case, dev)
    out, grads = _run(case, d, graph)
    v = dict(d)
    for name in ("x", "pos_src", "pos_dst"):
        flat = torch.zeros(d[name].numel() + 1, device=dev)
        flat[1:] = d[name].reshape(-1)
        v[name] = flat[1:].view(d[name].shape)
        assert v[name].data_ptr() % 16 != 0
    out_v, grads_v = _run(case, v, graph)
    assert torch.equal(out, out_v) and all(torch.equal(grads[k], grads_v[k]) for k in grads)
    _check(case, d, ref, out_v, grads_v)


def test_flow_target_to_source(dev):
    case = "tile edges"
    d, ei, ref = _found(case, dev)
    out, grads = _run(case, d, ei)
    flipped = _layer(case, d, flow="target_to_source")
    out_f, grads_f = _run(case, d, ei.flip(0).contiguous(), conv=flipped)
    assert torch.equal(out, out_f) and all(torch.equal(grads[k], grads_f[k]) for k in grads)
    _check(case, d, ref, out_f, grads_f)


def test_unsorted_edge_index_is_grouped(dev):
    case = "tile edges"
    d, ei, ref = _found(case, dev)
    out, grads = _run(case, d, ei)
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(3)).to(dev)
    out_p, grads_p = _run(case, d, ei[:, perm].contiguous())
    _close(out_p, ref.out, "shuffled edge index")                        # another entry order: the same maxima
    for k in grads:
        _close(grads_p[k], grads[k].cpu(), f"shuffled edge index g_{k}")


# ---- 2. routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["set abstraction", "one set", "tile edges"])
def test_poisoned_buffers(dev, case):
    d, graph, _ref = _found(case, dev)
    out, grads = _run(case, d, graph)
    for pattern in pa.PATTERNS:
        with pa.poisoned(pattern) as p:
            out_p, grads_p = _run(case, d, graph)
        assert p.count > 0, f"{case}: nothing was poisoned under {pattern!r}"
        assert pa.differing(out_p, out).numel() == 0, (case, pattern)
        for k in grads:
            assert pa.differing(grads_p[k], grads[k]).numel() == 0, (case, pattern, k)


def test_dmet_pointnet_0_takes_the_generic_route(dev, monkeypatch):
    from deepmetv2_amd import _native
    calls = []
    real = _native._pointnet_fwd
    monkeypatch.setattr(_native, "_pointnet_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for case in ("set abstraction", "one set"):
        d, graph, ref = _found(case, dev)
        del calls[:]
        out, grads = _run(case, d, graph)
        assert len(calls) == 1
        monkeypatch.setenv("DMET_POINTNET", "0")
        del calls[:]
        out_g, grads_g = _run(case, d, graph)
        assert len(calls) == 0
        monkeypatch.delenv("DMET_POINTNET")
        _check(case, d, ref, out_g, grads_g)
        _close(out_g, out.cpu(), f"{case}: generic against fused")
        for k in grads:
            _close(grads_g[k], grads[k].cpu(), f"{case}: generic against fused g_{k}")


def test_three_linear_local_nn_and_mean_and_autocast_take_the_generic_route(dev, monkeypatch):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    calls = []
    real = _native._pointnet_fwd
    monkeypatch.setattr(_native, "_pointnet_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    case = "set abstraction"
    d, graph, ref = _found(case, dev)
    c = pc.CASES[case]
    x, ps, pd = d["x"], d["pos_src"], d["pos_dst"]
    tgt, src, _code, _self = ref.tgt, ref.src, ref.code, ref.is_self
    feat = torch.cat([x.cpu().double()[src], ps.cpu().double()[src] - pd.cpu().double()[tgt]], dim=1)
    Nt = pd.shape[0]
    # a three-Linear local_nn
    torch.manual_seed(3)
    deep = torch.nn.Sequential(torch.nn.Linear(c["F"] + c["D"], 24), torch.nn.ReLU(), torch.nn.Linear(24, 24), torch.nn.ReLU(),
                               torch.nn.Linear(24, 16)).to(dev)
    out = dm.PointNetConv(deep, add_self_loops=False)((x, None), (ps, pd), graph)
    msg = deep.cpu().double()(feat).detach()
    want = torch.zeros(Nt, 16, dtype=torch.float64).scatter_reduce(0, tgt.view(-1, 1).expand_as(msg), msg, "amax",
                                                                   include_self=False)
    _close(out, want, "three Linears")
    # aggr = 'mean' over the fusable local_nn
    conv = _layer(case, d, aggr="mean")
    out = conv((x, None), (ps, pd), graph)
    deg = torch.bincount(tgt, minlength=Nt).clamp(min=1).double().view(-1, 1)
    want = torch.zeros(Nt, c["H2"], dtype=torch.float64).index_add_(0, tgt, ref.m) / deg
    _close(out, want, "aggr mean")
    # bf16 autocast: the generic route, at the bf16 bar (R6)
    conv = _layer(case, d)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = conv((x, None), (ps, pd), graph)
    assert out.dtype == torch.float32
    _close(out, ref.out, "bf16 autocast", BF16_BAR)
    assert len(calls) == 0
    # local_nn=None: the maximum of [x_j || pos_j - pos_i] itself
    out = dm.PointNetConv(add_self_loops=False)((x, None), (ps, pd), graph)
    want = torch.zeros(Nt, feat.shape[1], dtype=torch.float64).scatter_reduce(0, tgt.view(-1, 1).expand_as(feat), feat, "amax",
                                                                             include_self=False)
    _close(out, want, "local_nn=None")


def test_global_nn_and_pair_errors(dev):
    import deepmetv2_amd as dm
    case = "set abstraction"
    d, graph, ref = _found(case, dev)
    conv = _layer(case, d)
    conv.global_nn = torch.nn.Linear(pc.CASES[case]["H2"], 3).to(dev)
    out = conv((d["x"], None), (d["pos_src"], d["pos_dst"]), graph)
    want = conv.global_nn.cpu().double()(ref.out).detach()
    _close(out, want, "global_nn")
    with pytest.raises(ValueError, match="add_self_loops=False"):
        dm.PointNetConv(conv.local_nn)((d["x"], None), (d["pos_src"], d["pos_dst"]), graph)


def test_no_host_sync_over_a_padded_table(dev):
    import deepmetv2_amd as dm
    case = "set abstraction"
    c = pc.CASES[case]
    d = _to(pc.make_inputs(case, 0), dev)
    for b, counts in ((d["batch_src"], c["src"]), (d["batch_dst"], c["dst"])):
        ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(counts).cumsum(0)]).to(dev)
        dm.register_batch(b, ptr, len(counts), max_nodes=max(counts), min_nodes=min(counts))
    conv = _layer(case, d)
    x = d["x"].clone().requires_grad_(True)
    ps, pd = d["pos_src"].clone().requires_grad_(True), d["pos_dst"].clone().requires_grad_(True)
    g = _gout(case, dev)

    def step():
        table = dm.knn_xy_table(ps.detach(), pd.detach(), c["graph"][1], d["batch_src"], d["batch_dst"], batch_size=2)
        out = conv((x, None), (ps, pd), table)
        out.backward(g)
        return out
    step()                      # module loads, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out).all()) and bool(x.grad.abs().sum() > 0) and bool(ps.grad.abs().sum() > 0)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------
def _train(dev, seed):
    import deepmetv2_amd as dm
    torch.manual_seed(seed)
    sizes = [60, 55, 64]
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    batch = pc.batch_of(sizes).to(dev)
    pos = torch.randn(N, 2, generator=g).to(dev)
    x = torch.randn(N, 6, generator=g).to(dev)
    pxy = torch.randn(N, 2, generator=g).to(dev)
    truth = torch.randn(3, 2, generator=g).to(dev)
    conv = dm.PointNetConv(torch.nn.Sequential(torch.nn.Linear(8, 32), torch.nn.ReLU(), torch.nn.Linear(32, 32)),
                           add_self_loops=False).to(dev)
    head = torch.nn.Linear(32, 1).to(dev)
    params = list(conv.parameters()) + list(head.parameters())
    opt = torch.optim.SGD(params, lr=1e-2)
    losses = []
    for _ in range(3):
        idx = dm.fps(pos, batch, ratio=0.25, random_start=False)
        table = dm.radius_xy_table(pos, pos[idx], 1.0, batch, batch[idx], max_num_neighbors=16, batch_size=3)
        h = conv((x, None), (pos, pos[idx]), table)
        up = dm.knn_interpolate(h, pos[idx], pos, batch[idx], batch, k=3)
        w = head(up).view(-1)
        met = dm.met_reduce(w, pxy, batch, num_events=3)
        loss = ((met - truth) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, [p.detach().clone() for p in params]


def test_set_abstraction_chain_trains_and_repeats(dev):
    losses_a, params_a = _train(dev, 7)
    losses_b, params_b = _train(dev, 7)
    assert all(l == l and abs(l) != float("inf") for l in losses_a)
    assert losses_a == losses_b
    assert all(torch.equal(a, b) for a, b in zip(params_a, params_b))
    assert any(bool((p != 0).any()) for p in params_a)

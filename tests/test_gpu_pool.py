"""graclus / normalized_cut / cluster pooling / global pools / DynamicReductionNetwork on the GPU, against the CPU
restatement of include/dmet.h (tests/pool_reference.py) and torch compositions."""
import copy
import types

import numpy as np
import pytest
import torch

import pool_reference as ref

pytestmark = pytest.mark.gpu


def _ragged(sizes, D, seed):
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor(sizes, dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), counts)
    return torch.randn(int(ptr[-1]), D, generator=g), batch, ptr


def _knn_sym(dev, sizes, k, D, seed):
    import deepmetv2_amd as dm
    x, batch, ptr = _ragged(sizes, D, seed)
    xd, bd = x.to(dev), batch.to(dev)
    ei = dm.to_undirected(dm.knn_graph(xd, k, bd, loop=False), num_nodes=xd.shape[0])
    return xd, bd, ptr, ei


def _ref_graclus(ei, N, ptr, w, seed, max_rounds=0):
    rowptr, col, ws = ref.to_csr(ei.cpu().numpy(), N, None if w is None else w.cpu().numpy())
    c, p, _r = ref.graclus(rowptr, col, ws, ptr.numpy(), seed, max_rounds)
    return torch.from_numpy(c), torch.from_numpy(p)


def _partner(cluster):
    from deepmetv2_amd import pool
    from deepmetv2_amd.graph import _registry_get
    return _registry_get(pool._graclus_registry, cluster)


SIZES = [1, 2, 17, 500, 4500, 8000]


@pytest.mark.parametrize("weighted", [False, True])
def test_graclus_bit_exact_on_symmetrised_knn(dev, weighted):
    import deepmetv2_amd as dm
    xd, bd, ptr, ei = _knn_sym(dev, SIZES, 16, 64, seed=1)
    N = xd.shape[0]
    w = dm.normalized_cut_2d(ei, xd) if weighted else None
    cl = dm.graclus(ei, w, N, batch=bd, seed=77)
    c_ref, p_ref = _ref_graclus(ei, N, ptr, w, 77)
    assert torch.equal(cl.cpu(), c_ref)
    assert torch.equal(_partner(cl).cpu().long(), p_ref)
    ref.check_matching(c_ref.numpy(), p_ref.numpy(), ei.cpu().numpy(), ptr.numpy())
    # same seed -> same bits; batch passed / registered / omitted -> same bits
    assert torch.equal(dm.graclus(ei, w, N, batch=bd, seed=77), cl)
    b2 = bd.clone()
    dm.register_batch(b2, ptr.to(dev), len(SIZES))
    assert torch.equal(dm.graclus(ei, w, N, batch=b2, seed=77), cl)
    assert torch.equal(dm.graclus(ei, w, N, seed=77), cl)
    ei_plain = ei.clone()           # not tagged: sorted on the device, the whole graph matched as one block
    assert torch.equal(dm.graclus(ei_plain, w, N, seed=77), cl)
    assert not torch.equal(dm.graclus(ei, w, N, batch=bd, seed=78), cl)


def _radius_graph_loops_duplicates(dev):
    """(x, batch, ptr, edge_index): a radius graph with self loops, then unsorted, with 50 duplicated edges and every
    13th node isolated (all its edges dropped)."""
    import deepmetv2_amd as dm
    x, batch, ptr = _ragged([300, 40, 700], 2, seed=5)
    xd, bd = x.to(dev), batch.to(dev)
    ei = dm.radius_graph(xd, 0.3, bd, loop=True, max_num_neighbors=32)    # self loops present
    assert bool((ei[0] == ei[1]).any())
    keep = (ei[0] % 13 != 0) & (ei[1] % 13 != 0)
    ei = ei[:, keep]
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(0)).to(dev)
    return xd, bd, ptr, torch.cat([ei[:, perm], ei[:, :50]], 1)


def test_graclus_radius_graph_self_loops_isolated_ties(dev):
    import deepmetv2_amd as dm
    xd, bd, ptr, ei = _radius_graph_loops_duplicates(dev)
    N = xd.shape[0]
    for w in (None, torch.ones(ei.shape[1], device=dev)):           # unweighted, all-equal weights (tie rule)
        for mr in (0, 1, 2):
            cl = dm.graclus(ei, w, N, batch=bd, seed=3, max_rounds=mr)
            c_ref, p_ref = _ref_graclus(ei, N, ptr, w, 3, mr)
            assert torch.equal(cl.cpu(), c_ref), (w is None, mr)
            assert torch.equal(_partner(cl).cpu().long(), p_ref)
    iso = torch.arange(0, N, 13)
    assert torch.equal(cl.cpu()[iso], iso)


@pytest.mark.parametrize("max_rounds", [1, 2, 0])
def test_graclus_above_the_lds_cap_and_finisher(dev, max_rounds):
    import deepmetv2_amd as dm
    sizes = [20000, 300]
    assert sizes[0] > 16384        # DMET_GRACLUS_LDS_NODES: state in the workspace
    xd, bd, ptr, ei = _knn_sym(dev, sizes, 4, 3, seed=9)
    N = xd.shape[0]
    w = dm.normalized_cut_2d(ei, xd)
    cl = dm.graclus(ei, w, N, batch=bd, seed=11, max_rounds=max_rounds)
    c_ref, p_ref = _ref_graclus(ei, N, ptr, w, 11, max_rounds)
    assert torch.equal(cl.cpu(), c_ref)
    assert torch.equal(_partner(cl).cpu().long(), p_ref)


def test_graclus_no_host_sync_with_registered_batch(dev):
    import deepmetv2_amd as dm
    xd, bd, ptr, ei = _knn_sym(dev, [50, 300, 7], 8, 16, seed=2)
    N = xd.shape[0]
    dm.register_batch(bd, ptr.to(dev), 3, max_nodes=300, min_nodes=7)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = dm.normalized_cut_2d(ei, xd)
        cl = dm.graclus(ei, w, N, batch=bd)
        gm = dm.global_max_pool(xd, bd)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert cl.shape == (N,) and gm.shape == (3, 16)


def test_normalized_cut_vs_torch(dev):
    import deepmetv2_amd as dm
    for D in (2, 64):
        xd, bd, ptr, ei = _knn_sym(dev, [40, 300, 5], 8, D, seed=D)
        N = xd.shape[0]
        row, col = ei.cpu()
        deg = torch.bincount(col, minlength=N).to(torch.float32)
        inv = 1.0 / deg
        attr = torch.rand(ei.shape[1], generator=torch.Generator().manual_seed(1))
        want = attr * (inv[row] + inv[col])
        got = dm.normalized_cut(ei, attr.to(dev), N).cpu()
        torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
        x = xd.cpu().double()
        dist = (x[row] - x[col]).norm(dim=1).to(torch.float32)
        want2 = dist * (inv[row] + inv[col])
        got2 = dm.normalized_cut_2d(ei, xd).cpu()
        torch.testing.assert_close(got2, want2, rtol=1e-6, atol=0)


def _pool_reference(cluster, x, batch, mode):
    """torch composition on the CPU: consecutive ids, scatter_reduce, gradient to the lowest-index winner."""
    inv = torch.from_numpy(ref.consecutive(cluster.numpy()))
    C = int(inv.max()) + 1
    F = x.shape[1]
    idx = inv.view(-1, 1).expand(-1, F)
    if mode == "max":
        out = torch.zeros(C, F).scatter_reduce(0, idx, x, "amax", include_self=False)
        hit = x == out[inv]
        node = torch.arange(x.shape[0]).view(-1, 1).expand(-1, F)
        win = torch.full((C, F), x.shape[0]).scatter_reduce(0, idx, torch.where(hit, node, x.shape[0]), "amin")
        route = win[inv] == node
    else:
        out = torch.zeros(C, F).scatter_reduce(0, idx, x, "mean", include_self=False)
        route = None
    pb = torch.zeros(C, dtype=torch.int64).scatter_reduce(0, inv, batch, "amax", include_self=False)
    return out, route, inv, pb


@pytest.mark.parametrize("kind", ["graclus", "user", "ties"])
@pytest.mark.parametrize("mode", ["max", "mean"])
def test_pool_x_forward_backward(dev, kind, mode):
    import deepmetv2_amd as dm
    sizes = [60, 3, 250, 1]
    xd, bd, ptr, ei = _knn_sym(dev, sizes, 6, 8, seed=4)
    N = xd.shape[0]
    if kind == "user":
        # random, unsorted ids that stay inside an event (so the pooled batch is sorted and registered)
        g = torch.Generator().manual_seed(3)
        cl = torch.cat([lo * 10 + torch.randint(0, max(int(hi - lo) // 3, 1), (int(hi - lo),), generator=g) * 7
                        for lo, hi in zip(ptr[:-1], ptr[1:])])
        cld = cl.to(dev)
    else:
        cld = dm.graclus(ei, dm.normalized_cut_2d(ei, xd), N, batch=bd, seed=5)
        cl = cld.cpu()
    if kind == "ties":
        xd = torch.round(xd * 2) / 2          # many exact ties inside a pair
    x = xd.detach().cpu()
    out_ref, route, inv, pb_ref = _pool_reference(cl, x, bd.cpu(), mode)
    xg = xd.clone().requires_grad_(True)
    fn = dm.max_pool_x if mode == "max" else dm.avg_pool_x
    out, pb = fn(cld, xg, bd)
    gup = torch.randn(out.shape, generator=torch.Generator().manual_seed(8))
    out.backward(gup.to(dev))
    if mode == "max":
        assert torch.equal(out.detach().cpu(), out_ref)
        gx_ref = torch.where(route, gup[inv], torch.zeros_like(x))
        assert torch.equal(xg.grad.cpu(), gx_ref)
    else:
        torch.testing.assert_close(out.detach().cpu(), out_ref, rtol=1e-6, atol=1e-6)
        cnt = torch.bincount(inv).to(torch.float32)
        torch.testing.assert_close(xg.grad.cpu(), gup[inv] / cnt[inv].view(-1, 1), rtol=1e-6, atol=0)
    assert torch.equal(pb.cpu(), pb_ref)
    from deepmetv2_amd.graph import _batch_registry, _registry_get
    info = _registry_get(_batch_registry, pb)
    assert info is not None and info.num_events == len(sizes)
    counts = torch.bincount(pb_ref, minlength=len(sizes))
    assert torch.equal(info.ptr.cpu(), torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]))
    assert info.max_nodes == int(counts.max()) and info.min_nodes == int(counts.min())
    # the next graph build on the pooled nodes needs no host sync (self loops kept, every pooled event >= k nodes)
    if info.min_nodes >= 1:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            nxt = dm.knn_graph(out.detach(), 1, pb, loop=True)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert nxt.shape == (2, out.shape[0])


def test_global_pools(dev):
    import deepmetv2_amd as dm
    x, batch, ptr = _ragged([5, 0, 9, 1], 6, seed=6)
    xd, bd = x.to(dev).requires_grad_(True), batch.to(dev)
    B = 6            # two trailing empty events as well as the empty one inside
    idx = batch.view(-1, 1).expand(-1, 6)
    mx = torch.zeros(B, 6).scatter_reduce(0, idx, x, "amax", include_self=False)
    sm = torch.zeros(B, 6).index_add(0, batch, x)
    cnt = torch.bincount(batch, minlength=B).clamp(min=1).to(torch.float32).view(-1, 1)
    assert torch.equal(dm.global_max_pool(xd, bd, size=B).detach().cpu(), mx)
    torch.testing.assert_close(dm.global_add_pool(xd, bd, size=B).detach().cpu(), sm, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(dm.global_mean_pool(xd, bd, size=B).detach().cpu(), sm / cnt, rtol=1e-6, atol=1e-6)
    assert dm.global_max_pool(xd, bd).shape == (4, 6)       # the same tensor: size=B above is not remembered
    one = dm.global_mean_pool(xd, None)
    assert one.shape == (1, 6)
    torch.testing.assert_close(one.detach().cpu(), x.mean(0, keepdim=True), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dm.global_max_pool(xd, None).detach().cpu(), x.max(0, keepdim=True).values)
    dm.global_max_pool(xd, bd).sum().backward()
    g = torch.zeros_like(x)
    am = torch.stack([x[int(ptr[b]):int(ptr[b + 1])].argmax(0) + ptr[b] for b in (0, 2, 3)])
    for r in am:
        g[r, torch.arange(6)] = 1
    assert torch.equal(xd.grad.cpu(), g)


@pytest.mark.parametrize("sizes", [[30, 70], [300, 520]], ids=["30-70", "300-520"])     # inside / past one 256-node chunk
def test_max_pool_edge_coarsening(dev, sizes):
    import deepmetv2_amd as dm
    xd, bd, ptr, ei = _knn_sym(dev, sizes, 5, 4, seed=12)
    N = xd.shape[0]
    cl = dm.graclus(ei, None, N, batch=bd, seed=1)
    attr = torch.rand(ei.shape[1], 2, device=dev)
    pos = torch.randn(N, 3, device=dev)
    data = types.SimpleNamespace(x=xd, batch=bd, edge_index=ei, edge_attr=attr, pos=pos)
    out = dm.max_pool(cl, data)
    assert out is not data and data.x is xd
    inv = torch.from_numpy(ref.consecutive(cl.cpu().numpy()))
    sums = {}
    for (a, b), v in zip(ei.cpu().t().tolist(), attr.cpu().double()):
        a, b = int(inv[a]), int(inv[b])
        if a != b:
            sums[(a, b)] = sums.get((a, b), 0) + v
    keys = sorted(sums)
    assert out.edge_index.cpu().t().tolist() == [list(k) for k in keys]
    want = torch.stack([sums[k] for k in keys]).float()
    torch.testing.assert_close(out.edge_attr.cpu(), want, rtol=1e-5, atol=1e-6)
    pos_ref = torch.zeros(int(inv.max()) + 1, 3).scatter_reduce(0, inv.view(-1, 1).expand(-1, 3), pos.cpu(), "mean",
                                                                 include_self=False)
    torch.testing.assert_close(out.pos.cpu(), pos_ref, rtol=1e-6, atol=1e-6)
    x_ref, _r, _i, pb = _pool_reference(cl.cpu(), xd.cpu(), bd.cpu(), "max")
    assert torch.equal(out.x.cpu(), x_ref) and torch.equal(out.batch.cpu(), pb)
    # this package's Batch: ptr / max_nodes / min_nodes follow
    from deepmetv2_amd.data import Batch
    b = Batch(xd, torch.zeros(2, 1, device=dev), bd, ptr.to(dev), max(sizes), min_nodes=min(sizes))
    ob = dm.max_pool(cl, b)
    counts = torch.bincount(pb, minlength=2)
    assert torch.equal(ob.ptr.cpu(), torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]))
    assert ob.max_nodes == int(counts.max()) and ob.min_nodes == int(counts.min())
    assert ob.num_graphs == 2


# ---- the model ---------------------------------------------------------------------------------------------------------
def _drn_inputs(dev, sizes, input_dim=5, seed=0):
    x, batch, ptr = _ragged(sizes, input_dim, seed)
    return types.SimpleNamespace(x=x.to(dev), batch=batch.to(dev)), ptr


def _drn_by_hand(m, data, seeds, ops):
    """The DRN forward spelled out with the given operator set (public GPU operators, or CPU restatements)."""
    x = m.inputnet(m.datanorm * data.x)
    batch = data.batch
    for conv, s in zip((m.edgeconv1, m.edgeconv2), seeds):
        N = x.shape[0]
        ei = ops.to_undirected(ops.knn_graph(x, m.k, batch, loop=False), num_nodes=N)
        x = ops.edge_conv(conv, x, ei)
        w = ops.normalized_cut_2d(ei, x)
        cl = ops.graclus(ei, w, N, batch, s)
        x, batch = ops.max_pool_x(cl, x, batch)
    return m.output(ops.global_max_pool(x, batch)).squeeze(-1)


@pytest.mark.parametrize("sizes", [[40, 9, 60], [300, 9, 700]], ids=["40-9-60", "300-9-700"])
def test_drn_matches_hand_composition_and_cpu_restatement(dev, sizes):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    torch.manual_seed(0)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=16, k=4)
    m_cpu = copy.deepcopy(m)
    m_hand = copy.deepcopy(m).to(dev)
    m = m.to(dev)
    data, ptr = _drn_inputs(dev, sizes)
    seeds = (21, 22)
    out = m(data, seeds=seeds)
    out.sum().backward()

    gpu_ops = types.SimpleNamespace(
        to_undirected=dm.to_undirected, knn_graph=dm.knn_graph, edge_conv=lambda c, x, ei: c(x, ei),
        normalized_cut_2d=dm.normalized_cut_2d, graclus=lambda ei, w, N, b, s: dm.graclus(ei, w, N, batch=b, seed=s),
        max_pool_x=dm.max_pool_x, global_max_pool=dm.global_max_pool)
    out_h = _drn_by_hand(m_hand, data, seeds, gpu_ops)
    out_h.sum().backward()
    assert torch.equal(out.detach(), out_h.detach())
    for (n, p), ph in zip(m.named_parameters(), m_hand.parameters()):
        assert torch.equal(p.grad, ph.grad), n

    # fp32 torch / CPU composition that takes the GPU's cluster vectors
    clusters = []
    rec = types.SimpleNamespace(**vars(gpu_ops))
    rec.graclus = lambda ei, w, N, b, s: clusters.append(dm.graclus(ei, w, N, batch=b, seed=s).cpu()) or clusters[-1].to(dev)
    m_probe = copy.deepcopy(m_cpu).to(dev)
    _drn_by_hand(m_probe, data, seeds, rec)

    def cpu_pool(cl, x, batch):
        o, _r, inv, pb = _pool_reference(cl, x.detach(), batch, "max")
        idx = inv.view(-1, 1).expand(-1, x.shape[1])
        return torch.zeros_like(o).scatter_reduce(0, idx, x, "amax", include_self=False), pb

    it = iter(clusters)
    cpu_ops = types.SimpleNamespace(
        to_undirected=lambda ei, num_nodes: dm.to_undirected(ei, num_nodes),
        knn_graph=lambda x, k, b, loop: ref_ops.knn_graph(x.detach(), k, b, loop=loop),
        edge_conv=lambda c, x, ei: ref_ops.edge_conv(x, ei, c.nn, c.aggr),
        normalized_cut_2d=lambda ei, x: None, graclus=lambda ei, w, N, b, s: next(it),
        max_pool_x=cpu_pool,
        global_max_pool=lambda x, b: torch.zeros(3, x.shape[1]).scatter_reduce(
            0, b.view(-1, 1).expand(-1, x.shape[1]), x, "amax", include_self=False))
    data_cpu = types.SimpleNamespace(x=data.x.cpu(), batch=data.batch.cpu())
    out_c = _drn_by_hand(m_cpu, data_cpu, seeds, cpu_ops)
    out_c.sum().backward()
    torch.testing.assert_close(out.detach().cpu(), out_c.detach(), rtol=1e-4, atol=1e-5)
    # relative to the gradient scale of the parameter's own layer: the bias in front of ELU + BatchNorm has a gradient
    # that nearly cancels (BatchNorm removes the channel mean), so its own magnitude is no yardstick
    scale = {}
    for n, pc in m_cpu.named_parameters():
        layer = n.rsplit(".", 1)[0]
        scale[layer] = max(scale.get(layer, 0.0), float(pc.grad.abs().max()))
    for (n, p), pc in zip(m.named_parameters(), m_cpu.parameters()):
        tol = 1e-4 * max(scale[n.rsplit(".", 1)[0]], 1e-6)
        err = float((p.grad.cpu() - pc.grad).abs().max())
        assert err <= tol + 1e-4 * float(pc.grad.abs().max()), (n, err, tol, float(pc.grad.abs().max()))


def test_drn_full_size(dev):
    import deepmetv2_amd as dm
    torch.manual_seed(1)
    m = dm.DynamicReductionNetwork(input_dim=5, hidden_dim=64, k=16).to(dev)
    data, ptr = _drn_inputs(dev, [4500] * 64, seed=3)
    dm.register_batch(data.batch, ptr.to(dev), 64, max_nodes=4500, min_nodes=4500)
    out = m(data)
    out.sum().backward()
    assert out.shape == (64,) and bool(torch.isfinite(out).all())
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n

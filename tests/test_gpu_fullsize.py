"""GPU parity at BASELINE.json's full sizes and on adversarial kNN inputs (HIP path through the C ABI vs the CPU oracle).

* configs[1]: the whole `Net(dynamic, k=16)` training step on 64 events x 4500 nodes against `oracle/ref_model.RefNet`
  on the SAME 64 events (train-mode BatchNorm statistics are over the whole batch, so a subset would not do): per-node
  weights, per-event MET, loss, gradients.  Reference call sites: model/graph_met_network.py:63, train.py:48-51.
* configs[4]: DynamicEdgeConv forward / backward on a ragged batch with events of 5120..8000 nodes (too large for the
  LDS-resident gather: L2-form gather, multi-pass backward scatter) against `ref_ops.dynamic_edge_conv`.
* kNN matrix-core filter (both forms: events below / above 800 nodes, csrc/knn.hip kF2MinNodes; the filter is csrc/knn_filter.h) on inputs built to break it: non-finite rows,
  coordinates whose distances exceed the 1e10 sentinel, per-feature heavy tails, a large common offset, mirrored pairs
  that tie to the last ulp.  The result must still be the C oracle's bits; where the certificate cannot hold, the
  exact fallback must have run (flagged_queries > 0).
"""
import os

import pytest
import torch

F2_MIN_NODES = 800     # csrc/knn.hip kF2MinNodes: smallest event the second filter form (fp16 tile records) takes
pytestmark = pytest.mark.gpu


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


class _ForcedGraphConv(torch.nn.Module):
    """Oracle EdgeConv over a given edge_index (keeps the caller's `nn` under `.nn`, like RefEdgeConv)."""

    def __init__(self, nn_module, edge_index):
        super().__init__()
        self.nn, self.edge_index = nn_module, edge_index

    def forward(self, x, _graph_arg=None):
        from oracle import ref_ops
        return ref_ops.edge_conv(x, self.edge_index, self.nn, "max", "source_to_target")


def test_config1_full_train_step_matches_oracle(dev, monkeypatch):
    """BASELINE configs[1] at full size: forward + loss + backward of the 2-layer dynamic model on all 64 events.

    Bit-exact kNN indices are a property of identical inputs, and the second layer's kNN runs on an embedding that
    differs from a CPU run's by ~1e-6 (fused kernels reassociate), so a run-to-run comparison of whole models is
    undefined on near-ties at rank k (hard part 1).  The test therefore pins the path stage by stage:
      1. each layer's kNN table (captured from the HIP run) == the C oracle's on the SAME embedding the HIP run fed it;
      2. the oracle model, made to convolve over exactly those graphs, must then agree on per-node weights, per-event
         MET, loss and gradients within the fp32 bars."""
    import deepmetv2_amd.conv as conv_mod
    from deepmetv2_amd import register_batch, synth
    from deepmetv2_amd.model import Net, loss_fn, split_features
    from deepmetv2_amd.scatter import met_reduce
    from oracle import ref_model, ref_ops

    B, n, k = 64, 4500, 16
    x, y, batch, ptr = synth.make_events([n] * B, seed=2024)
    torch.manual_seed(3)
    model = Net(8, 3, graph="dynamic", k=k)
    ref = ref_model.RefNet(8, 3, graph="dynamic", k=k)
    ref.load_state_dict(model.state_dict())
    model = model.to(dev).train()
    ref = ref.train()

    captured = []
    real_knn_table = conv_mod.knn_table

    def spy(xx, kk, bb=None, loop=True, **kw):
        t = real_knn_table(xx, kk, bb, loop=loop, **kw)
        captured.append((xx.detach().cpu(), t.nbr.cpu(), t.dist.cpu()))
        return t

    monkeypatch.setattr(conv_mod, "knn_table", spy)
    # builds that carried the BatchNorm transform of the block before (dmet_bn_knn_local_dense_f32) hand their table over
    # through DynamicEdgeConv._take_prebuilt instead of knn_table
    real_take = conv_mod.DynamicEdgeConv._take_prebuilt

    def spy_take(self, xx):
        t = real_take(self, xx)
        if t is not None:
            captured.append((xx.detach().cpu(), t.nbr.cpu(), t.dist.cpu()))
        return t

    monkeypatch.setattr(conv_mod.DynamicEdgeConv, "_take_prebuilt", spy_take)
    xd, yd, bd, pd = x.to(dev), y.to(dev), batch.to(dev), ptr.to(dev)
    register_batch(bd, pd, B, max_nodes=n)
    w = model(*split_features(xd), None, bd)
    loss = loss_fn(w, xd, yd, bd, ptr=pd)
    loss.backward()
    met = met_reduce(w.detach(), xd, ptr=pd).cpu()
    assert len(captured) == 2

    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    tgt = torch.arange(B * n, dtype=torch.int64).view(-1, 1).expand(-1, k).reshape(-1)
    for layer, (emb, nbr, dist) in enumerate(captured):
        nbr_ref, dist_ref = ref_ops.knn_table(emb, ptr, k)                       # 1. same input -> same bits
        assert torch.equal(nbr, nbr_ref) and torch.equal(dist, dist_ref), f"layer {layer}"
        assert int((nbr < 0).sum()) == 0
        ei = torch.stack([nbr.reshape(-1).long(), tgt])                          # [0] = source j, [1] = target i
        ref.graphnet.conv_continuous[layer][0] = _ForcedGraphConv(ref.graphnet.conv_continuous[layer][0].nn, ei)

    w_ref = ref(*split_features(x), None, batch)                                 # 2. same graphs
    loss_ref = ref_ops.loss_fn(w_ref, x, y, batch)
    loss_ref.backward()
    met_ref = ref_ops.met_sums_f64(w_ref.detach(), x, ptr)

    torch.testing.assert_close(w.detach().cpu(), w_ref.detach(), rtol=2e-4, atol=2e-5)
    # MET px / py per event: relative 1e-5 of sum |w p|
    wp = w_ref.detach().double().abs().view(-1, 1) * x[:, :2].double().abs()
    per_event = torch.zeros(B, 2, dtype=torch.float64).index_add_(0, batch, wp)
    assert bool(((met.double() - met_ref.double()).abs() <= 1e-5 * per_event + 1e-6).all())
    torch.testing.assert_close(loss.detach().cpu().view(()), loss_ref.detach().view(()), rtol=1e-4, atol=1e-3)
    # (the EdgeConv biases are followed by a train-mode BatchNorm: their true gradient is zero and both sides hold
    # rounding noise only, so they are not compared)
    for name in ("graphnet.conv_continuous.0.0.nn.0.weight", "graphnet.conv_continuous.1.0.nn.0.weight",
                 "graphnet.conv_continuous.1.1.weight", "graphnet.output.2.weight",
                 "graphnet.embed_continuous.0.weight", "graphnet.bn_all.weight"):
        g = dict(model.named_parameters())[name].grad.cpu()
        gr = dict(ref.named_parameters())[name].grad
        torch.testing.assert_close(g, gr, rtol=5e-3, atol=5e-4 * float(gr.abs().max()), msg=lambda m: f"{name}: {m}")


def test_config5_edgeconv_on_oversized_events_matches_oracle(dev):
    """BASELINE configs[4] sizes: events of 5120..8000 nodes next to small ones.  Forward, arg-max routing and all
    three gradients of DynamicEdgeConv(Linear(64, 32), k=16) against the PyG-shaped oracle."""
    import deepmetv2_amd as dm
    from oracle import ref_ops

    sizes = [8000, 5200, 600, 4500, 7000, 5119, 5120]
    H, k = 32, 16
    g = torch.Generator().manual_seed(17)
    N = sum(sizes)
    x = torch.randn(N, H, generator=g)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ptr = _ptr(sizes)
    lin = torch.nn.Sequential(torch.nn.Linear(2 * H, H))
    conv = dm.DynamicEdgeConv(nn=lin, k=k)        # (the constructor re-initialises `nn`, like PyG's: build it first)
    xr = x.clone().requires_grad_(True)
    out_ref = ref_ops.dynamic_edge_conv(xr, batch, lin, k)
    gup = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(1))
    out_ref.backward(gup)
    gW_ref, gb_ref, gx_ref = lin[0].weight.grad.clone(), lin[0].bias.grad.clone(), xr.grad.clone()
    lin.zero_grad()

    conv = conv.to(dev)
    bd = batch.to(dev)
    dm.register_batch(bd, ptr.to(dev), len(sizes), max_nodes=max(sizes))
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, bd)
    out.backward(gup.to(dev))
    torch.testing.assert_close(out.detach().cpu(), out_ref.detach(), rtol=1e-5, atol=1e-5)
    # gx: the gradient of a maximum goes to ONE winning neighbour per (node, channel).  The fused path compares
    # W2.x_j, the oracle W.[x_i || x_j - x_i] + b: two messages that agree to the last ulp can swap places, which moves
    # one routed term W2[c,:] g[i,c] from node j to node j' (both are exact ties for R4's purposes).  So: nearly all
    # rows equal, and the routed mass is conserved column by column.
    scale = float(gx_ref.abs().max())
    gx = xd.grad.cpu()
    bad_rows = ((gx - gx_ref).abs() > 1e-5 * max(scale, 1.0) + 1e-4 * gx_ref.abs()).any(1)
    assert int(bad_rows.sum()) <= 1e-3 * N, int(bad_rows.sum())
    torch.testing.assert_close(gx[~bad_rows], gx_ref[~bad_rows], rtol=1e-4, atol=1e-5 * max(scale, 1.0))
    col_scale = gx_ref.double().abs().sum(0)
    assert bool(((gx.double().sum(0) - gx_ref.double().sum(0)).abs() <= 1e-5 * col_scale).all())
    # a swapped tie also moves g[i,c] (x_j' - x_j) inside row c of the W2 half of gW: allow a few of those
    # (the operator-level test below pins the backward kernels exactly, with the routing fixed)
    n_flip = max(1, int(bad_rows.sum()))
    torch.testing.assert_close(lin[0].weight.grad.cpu(), gW_ref, rtol=2e-4,
                               atol=2e-5 * float(gW_ref.abs().max()) + n_flip * float(gup.abs().max()) * 0.5)
    torch.testing.assert_close(lin[0].bias.grad.cpu(), gb_ref, rtol=2e-4, atol=2e-5 * float(gb_ref.abs().max()))


def test_config5_gather_kernels_on_oversized_events_exact(dev):
    """The kernels behind the test above, with the arg-max routing taken from the forward kernel itself so that nothing
    depends on how a tie resolves: L2-form gather + max (events > 5119 nodes cannot use the LDS image) against torch
    on the same P / Q tables, validity of `arg` (it IS a maximum, lowest slot among exact ties: R4), and the multi-pass
    LDS scatter of the backward against an index_add with the same routing."""
    from deepmetv2_amd import _native
    sizes = [8000, 5200, 600, 4500, 7000, 5119, 5120]
    H, k = 32, 16
    g = torch.Generator().manual_seed(23)
    N = sum(sizes)
    x = torch.randn(N, H, generator=g)
    W = torch.randn(H, 2 * H, generator=g) / 8.0
    b = torch.randn(H, generator=g)
    ptr = _ptr(sizes)
    xd, pd = x.to(dev), ptr.to(dev)
    nbr, _dist, loc = _native.knn_local(xd, pd, k)
    P, Q = _native.node_linear_split(xd, W.to(dev), b.to(dev), sliced=False)
    out, arg = _native.gather_max(P, Q, nbr, pd, want_arg=True, lds=False)
    Pc, Qc, nb = P.cpu(), Q.cpu(), nbr.cpu().long()
    msgs = Qc[nb]                                               # [N, k, H]
    best, first = msgs.max(1)                                   # torch returns the first maximum: lowest slot
    assert torch.equal(out.cpu(), Pc + best)
    assert torch.equal(arg.cpu().long(), first)
    g_out = torch.randn(N, H, generator=g)
    gQ = _native.gather_max_bwd_lds(g_out.to(dev), arg, nbr, pd, nbr_local=loc).cpu()
    src = nb.gather(1, first)                                   # [N, H]: winning source node per (node, channel)
    ref = torch.zeros(N, H, dtype=torch.float64)
    ref.view(-1).index_add_(0, (src * H + torch.arange(H)).view(-1), g_out.double().view(-1))
    # every term is rounded once to 2^-30 of the slice's max |g| (integer LDS sums): absolute bar from the in-degree
    indeg = torch.zeros(N).index_add_(0, nb.view(-1), torch.ones(N * k))
    tol = float(g_out.abs().max()) * 2.0 ** -29 * float(indeg.max()) * H + 1e-6
    assert float((gQ.double() - ref).abs().max()) <= tol + 1e-6 * float(ref.abs().max())


def _knn_vs_oracle(dev, x, sizes, k):
    from deepmetv2_amd import _native
    from oracle import ref_ops
    ptr = _ptr(sizes)
    nbr_ref, dist_ref = ref_ops.knn_table(x, ptr, k)
    st = {}
    nbr, dist, _loc = _native.knn_local(x.to(dev), ptr.to(dev), k, stats=st)
    nbr, dist = nbr.cpu(), dist.cpu()
    bad = (nbr != nbr_ref).any(1).nonzero().view(-1)
    assert bad.numel() == 0, f"{bad.numel()} rows differ, first {bad[:5].tolist()}, stats {st}"
    # distances bit for bit (NaN never appears in a result: candidates at NaN distance are not neighbours)
    assert torch.equal(dist, dist_ref), st
    return st


@pytest.mark.parametrize("D", [32, 64, "32-first-form"])
@pytest.mark.parametrize("sizes", [[2500, 700], [1300, 900, 600], [4500]])
@pytest.mark.parametrize("case", ["nonfinite_rows", "beyond_sentinel", "feature_tails", "common_offset",
                                  "mirrored_ulp_ties", "tight_far_cluster"])
def test_knn_filter_adversarial(dev, monkeypatch, case, sizes, D):
    """Matrix-core filter + certificate on hostile inputs, events on both sides of the 800-node switch between the
    two filter forms (kF2MinNodes; 2048 until round 3), at the model's width (32) and the DRN's (64: second form only,
    exact kernel for the rest).  Bits
    must equal the C oracle's (dmet_oracle.c:62: a candidate at d >= 1e10 or NaN is never a neighbour, short results
    are -1 / 1e10)."""
    if D == "32-first-form":
        # every event through the first filter form: with [4500] alone all its tiles are split tail tiles, i.e. the
        # sub-sweep merge of knn_rerank_kernel decides every row (found there: candidates at >= 1e10 were ranked)
        monkeypatch.setenv("DMET_KNN_FILTER", "1")
        D = 32
    filter_runs = (os.environ.get("DMET_KNN_PATH", "") != "exact"
                   and not (D == 64 and os.environ.get("DMET_KNN_FILTER", "") == "1"))   # 64 features: second form only
    seeds = {"nonfinite_rows": 11, "beyond_sentinel": 12, "feature_tails": 13, "common_offset": 14,
             "mirrored_ulp_ties": 15, "tight_far_cluster": 16}
    g = torch.Generator().manual_seed(seeds[case] * 10 + len(sizes) + D)
    N, k = sum(sizes), 16
    x = torch.randn(N, D, generator=g)
    expect_fallback = False
    if case == "nonfinite_rows":
        idx = torch.randperm(N, generator=g)[:40]
        x[idx[:10], 3] = float("nan")
        x[idx[10:20], 7] = float("inf")
        x[idx[20:30], 0] = float("-inf")
        x[idx[30:40]] = float("nan")
    elif case == "beyond_sentinel":
        # rows ~1e5..1e6 from the origin: their distances to everything (and, among the far ones, to each other unless
        # they coincide) are >= 1e10 and must come back as -1
        idx = torch.randperm(N, generator=g)[: N // 50]
        x[idx] = x[idx] * torch.empty(idx.numel(), 1).uniform_(1e5, 1e6, generator=g)
        x[idx[:4]] = x[idx[0]].clone()  # exact duplicates far away: distance 0 to each other, >= 1e10 to the rest
    elif case == "feature_tails":
        x = x * torch.exp(4.0 * torch.randn(1, D, generator=g))
    elif case == "common_offset":
        x = x + 100.0                   # neighbour distances ~1e-4 of the squared norms
    elif case == "mirrored_ulp_ties":
        # pairs placed symmetrically around a query, norms >> distances: equal in exact arithmetic, 0-2 ulp apart in
        # the fp32 chain; enough pairs per query to straddle rank k
        x = 0.01 * x + 40.0
        step = 97
        for q in range(5, N - 40, step):
            v = 0.002 * torch.randn(12, D, generator=g)
            x[q + 1:q + 13] = x[q] + v
            x[q + 13:q + 25] = x[q] - v
        expect_fallback = True
    elif case == "tight_far_cluster":
        c = 30.0 * torch.randn(6, D, generator=g)
        x = c[torch.randint(0, 6, (N,), generator=g)] + 1e-3 * x
        expect_fallback = True
    st = _knn_vs_oracle(dev, x.contiguous(), sizes, k)
    if expect_fallback and filter_runs:
        assert st["flagged_queries"] > 0, st     # the certificate cannot hold here: the exact fallback must have run
    if case == "feature_tails" and filter_runs:
        # (at 64 features the events below the second form's 800 nodes are handed to the exact kernel wholesale)
        by_design = sum(n for n in sizes if n < F2_MIN_NODES) if D == 64 else 0
        # The second filter form's operands are fp16: a row with a feature at or beyond 16384 is a forced candidate of
        # every query (and as a query goes to the exact path).  exp(4 randn) per feature puts most rows there, so the
        # second-form events of this case are recomputed exactly BY DESIGN (a stated limit of the fp16 records, DESIGN
        # K1); first-form events (bf16 split, full fp32 range) must still be certified.
        second_form = os.environ.get("DMET_KNN_FILTER", "") != "1"
        wide = bool((x.abs() >= 16384).any())
        for n in sizes:
            if second_form and wide and n >= F2_MIN_NODES:
                by_design += n
        assert st["flagged_queries"] - min(by_design, N) <= N // 20, st


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("case", ["fp16_subnormal_operands", "few_rows_beyond_fp16", "unit_scale_certified"])
def test_knn_fp16_operand_range(dev, case, D):
    """The second filter form ranks pairs with single-term fp16 operands (DESIGN K1, second session of round 2); its
    certificate assumes (a) round-to-nearest fp16 with subnormals KEPT by v_mfma_f32_32x32x16_f16 -- inputs of ~3e-5 are
    all subnormal in fp16: a flush would zero every product, every key would be |x_j|^2 and the wrong neighbours would be
    certified -- and (b) that rows with |v| >= 16384 are forced candidates rather than overflowed products.  Bits must
    equal the C oracle's in all cases; at unit scale (and with a handful of rows beyond the range) nearly every query
    must be certified by the filter itself."""
    g = torch.Generator().manual_seed(77 + D)
    sizes = [4500, 2300]
    N, k = sum(sizes), 16
    x = torch.randn(N, D, generator=g)
    if case == "fp16_subnormal_operands":
        x = x * 3.0e-5
    elif case == "few_rows_beyond_fp16":
        idx = torch.randperm(N, generator=g)[:5]
        x[idx, 3] = torch.tensor([2.0e4, -3.0e4, 1.7e4, 6.6e4, -7.0e4])   # still far below the 1e10 distance sentinel for most
    st = _knn_vs_oracle(dev, x.contiguous(), sizes, k)
    if os.environ.get("DMET_KNN_PATH", "") != "exact" and os.environ.get("DMET_KNN_FILTER", "") != "1":
        if case == "unit_scale_certified":
            assert st["flagged_queries"] <= 2, st
        elif case == "few_rows_beyond_fp16":
            assert st["flagged_queries"] <= 5 + 2, st       # the five rows themselves (as queries) + slack
        else:
            # most queries must have been certified from the subnormal operands themselves (the fallback would hide a flush)
            assert st["flagged_queries"] <= N // 4, st


def test_knn_many_sparse_uncertified_queries(dev):
    """More flagged queries than the per-query fallback has workgroups (512), at most a few per 128-query tile: clusters
    of 40 exact duplicates scattered over 8 events -- every member has 39 neighbours at distance 0, more ties at the
    threshold than the filter keeps, so its certificate fails and the list-driven fallback (the leading workgroups of
    the exact kernel's launch, each walking the list with a stride) recomputes it.  Bits equal the C oracle's."""
    g = torch.Generator().manual_seed(991)
    sizes = [4500] * 8
    N, D, k = sum(sizes), 32, 16
    x = torch.randn(N, D, generator=g)
    for c in range(40):
        ev = c % len(sizes)
        rows = ev * 4500 + torch.randperm(4500, generator=g)[:40]
        x[rows] = x[rows[0]].clone()
    st = _knn_vs_oracle(dev, x.contiguous(), sizes, k)
    if os.environ.get("DMET_KNN_PATH", "") != "exact":
        assert st["flagged_queries"] > 512, st           # (about half of the 1 600 duplicates: the rest certify)
        assert st["flagged_queries"] <= N // 10, st      # sparse: the rest of the batch stays certified


def test_knn_second_filter_form_paths_agree_fuzz(dev, monkeypatch):
    """Events of 800..7000 nodes (second filter form: whole sweeps, split tail tiles of a small batch, and the small
    events whose tail is never split) against the exact kernel on gaussian / clustered-with-duplicates / heavy-tailed /
    rank-2 data, k in {16, 8, 20, 13, 1}."""
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(4242)
    for it in range(12):
        B = int(torch.randint(1, 5, (1,), generator=g))
        lo_n = 2048 if it < 8 else F2_MIN_NODES                                 # the last rounds: small second-form events
        sizes = [int(v) for v in torch.randint(lo_n, 7000 if it < 8 else 2600, (B,), generator=g)]
        if it % 3 == 0:
            sizes.append(int(torch.randint(1, F2_MIN_NODES, (1,), generator=g)))       # a first-form event in the same batch
        N = sum(sizes)
        k = [16, 8, 20, 13, 1][it % 5]
        x = torch.randn(N, 32, generator=g)
        mode = it % 4
        if mode == 1:
            c = torch.randn(7, 32, generator=g) * 3
            x = c[torch.randint(0, 7, (N,), generator=g)] + 1e-2 * torch.randn(N, 32, generator=g)
            x[N // 2:N // 2 + N // 10] = x[:N // 10]
        elif mode == 2:
            x = x * torch.exp(2.0 * torch.randn(N, 1, generator=g))
        elif mode == 3:
            x = torch.randn(N, 2, generator=g) @ torch.randn(2, 32, generator=g)
        ptr = _ptr(sizes).to(dev)
        xd = x.to(dev)
        monkeypatch.setenv("DMET_KNN_PATH", "exact")
        n0, d0 = _native.knn(xd, ptr, k)
        monkeypatch.delenv("DMET_KNN_PATH")
        st = {}
        n1, d1, _ = _native.knn_local(xd, ptr, k, stats=st)
        assert torch.equal(n0, n1) and torch.equal(d0, d1), (it, sizes, k, mode, st)
        monkeypatch.setenv("DMET_KNN_FILTER", "1")       # first form on the same (large) events
        n2, d2 = _native.knn(xd, ptr, k)
        monkeypatch.delenv("DMET_KNN_FILTER")
        assert torch.equal(n0, n2) and torch.equal(d0, d2), (it, sizes, k, mode, "first form")


@pytest.mark.parametrize("D", [32, 64])
def test_knn_filter_form_boundaries(dev, monkeypatch, D):
    """Event sizes on both sides of every switch of the matrix-core path -- 799 / 800 / 801 nodes (first vs second
    filter form; exact kernel vs second form at 64 features), 2559 / 2560 / 2561 (smallest event whose tail sweeps are
    cut in two) and 65535 / 65536 / 65537 nodes (16-bit candidate ids, the second form's upper limit) -- against the
    exact kernel."""
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(700 + D)
    for sizes in ([799, 800, 801, 31], [2047, 2048, 2049, 31], [2559, 2560, 2561], [2560, 2600], [703, 704, 705],
                  [65535], [65536, 5], [65537]):
        N = sum(sizes)
        x = torch.randn(N, D, generator=g).to(dev)
        ptr = _ptr(sizes).to(dev)
        monkeypatch.setenv("DMET_KNN_PATH", "exact")
        n0, d0 = _native.knn(x, ptr, 16)
        monkeypatch.delenv("DMET_KNN_PATH")
        st = {}
        n1, d1 = _native.knn(x, ptr, 16, stats=st)
        assert torch.equal(n0, n1) and torch.equal(d0, d1), (sizes, st)


def test_knn_many_tiny_events(dev):
    """More events than the launch plans rank by size (4096): 5000 events of 0..40 nodes, every row against the C oracle
    (events shorter than k yield short rows padded with -1 / 1e10)."""
    g = torch.Generator().manual_seed(9)
    sizes = [int(v) for v in torch.randint(0, 41, (5000,), generator=g)]
    x = torch.randn(sum(sizes), 32, generator=g)
    _knn_vs_oracle(dev, x, sizes, 16)


def test_config2_bf16_edge_mlp_at_full_event_size(dev):
    """BASELINE configs[2] at the benchmark's event size (4 events x 4500 nodes, k = 16; round 2's largest bf16 case was
    1 300 nodes): the DynamicEdgeConv with its dense layer on the bf16 matrix cores and the bf16 Q table -- the build
    carrying that dense layer (layout 2 of dmet_knn_local_dense_f32), the bf16 gather -- against the fp32 oracle at the R6
    bf16 bar (features rtol 2e-2 of the output scale), the graph bit-exact, MET-style event sums within 1e-2 relative,
    gradients through the winners the bf16 table selected within 2e-2 relative (norm) of the fp32 oracle's where the
    winners agree, and tight against a torch emulation of the same bf16 recipe."""
    import deepmetv2_amd as dm
    from oracle import ref_ops
    H, k, sizes = 32, 16, [4500, 4500, 4500, 4500]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(sum(sizes), H, generator=g)
    ptr = _ptr(sizes)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    lin = torch.nn.Sequential(torch.nn.Linear(2 * H, H))
    conv = dm.DynamicEdgeConv(nn=lin, k=k)
    conv.compute_dtype = torch.bfloat16
    W, b = lin[0].weight.detach().clone(), lin[0].bias.detach().clone()
    xr = x.clone().requires_grad_(True)
    out_ref = ref_ops.dynamic_edge_conv(xr, batch, lin, k)
    gup = torch.randn(out_ref.shape, generator=g)
    out_ref.backward(gup)
    gW_ref = lin[0].weight.grad.clone()
    lin.zero_grad()
    conv = conv.to(dev)
    xd, bd, pd = x.to(dev).requires_grad_(True), batch.to(dev), ptr.to(dev)
    dm.register_batch(bd, pd, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    out = conv(xd, bd)
    out.backward(gup.to(dev))
    o = out.detach().cpu()
    scale = float(out_ref.abs().max())
    torch.testing.assert_close(o, out_ref.detach(), rtol=2e-2, atol=2e-2 * scale)
    # typical error far below the bar: bf16 operands (2^-9 relative) over 64-term products
    assert float((o - out_ref.detach()).abs().median()) < 2e-3 * scale
    # per-event sums of the features (the shape of the MET reduction): 1e-2 relative of the absolute sums
    ev = torch.zeros(len(sizes), H).index_add_(0, batch, o - out_ref.detach())
    ev_abs = torch.zeros(len(sizes), H).index_add_(0, batch, out_ref.detach().abs())
    assert bool((ev.abs() <= 1e-2 * ev_abs).all())
    # the same recipe in torch on the oracle's graph: only accumulation order and rare bf16 rounding flips of Q differ
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    xb = bf(x)
    Pe = xb @ bf(W[:, :H] - W[:, H:]).t() + b
    Qe = bf(xb @ bf(W[:, H:]).t())
    nbr, _ = ref_ops.knn_table(x, ptr, k)
    emu = Pe + Qe[nbr.long()].max(dim=1).values
    torch.testing.assert_close(o, emu, rtol=1e-2, atol=1e-2 * float(emu.abs().max()) * 2 ** -6)
    assert float((o - emu).abs().median()) < 1e-5 * max(1.0, float(emu.abs().max()))
    # gradients: fp32 arithmetic routed through the winners the bf16 table selected (straight-through over the roundings):
    # tight against exactly that emulation (lowest slot on ties), bounded against the fp32 oracle, whose near-ties the
    # bf16 rounding of Q decides differently (a routing difference, not an arithmetic one)
    gq = Qe[nbr.long()]
    slot = (gq == gq.max(dim=1, keepdim=True).values).float().argmax(dim=1)
    src = torch.gather(nbr.long(), 1, slot)
    gQ = torch.zeros_like(Qe).scatter_add_(0, src, gup)
    gWd, gW2 = gup.t() @ x, gQ.t() @ x
    gW_emu = torch.cat([gWd, gW2 - gWd], dim=1)
    relw = float((lin[0].weight.grad.cpu() - gW_emu).norm() / gW_emu.norm())
    assert relw < 2e-2, relw
    assert float((lin[0].weight.grad.cpu() - gW_ref).norm() / gW_ref.norm()) < 0.5

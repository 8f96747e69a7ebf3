"""The kernels of csrc/pool.hip at their edges, bit for bit against the CPU restatement of include/dmet.h
(tests/pool_reference.py): the pair-pool index past one 256-node chunk and past one 256-event scan chunk and over empty
events; pair pooling forward and backward over ties, signed zeros, infinities and every output combination; graclus on
directed rows, on rows with entries it must ignore, at the LDS cap, on many tiny blocks and under tied, negative and
infinite weights; the normalized cut on inputs whose result is exact.

Every comparison is exact (torch.equal, or the bits where signed zeros matter; NaNs match each other whatever their
payload), except the one general normalized-cut case, whose tolerance is derived where it is used."""
import functools
import types

import numpy as np
import pytest
import torch

import pool_reference as ref
from test_gpu_pool import _knn_sym, _partner, _pool_reference, _radius_graph_loops_duplicates, _ragged, _ref_graclus

pytestmark = pytest.mark.gpu

SHARES = [0.0, 0.3, 1.0]
POOL_SIZES = [257, 0, 513, 1]


def _same_bits(got: torch.Tensor, want) -> bool:
    """Bit equality of float32 values; NaNs match each other whatever their payload or sign."""
    got = got.detach().cpu().contiguous()
    want = torch.as_tensor(want).contiguous()
    if got.shape != want.shape or got.dtype != torch.float32 or want.dtype != torch.float32:
        return False
    ng, nw = got.isnan(), want.isnan()
    return torch.equal(ng, nw) and torch.equal(got.view(torch.int32)[~ng], want.view(torch.int32)[~nw])


@functools.lru_cache(maxsize=None)
def _matching(name, share):
    sizes = POOL_SIZES if name == "pool" else ref.index_cases()[name]
    ptr = ref.ptr_of(sizes)
    partner = ref.random_matching(ptr, np.random.default_rng(11), share)
    cid, pooled_ptr = ref.pair_index(partner, ptr)
    return ptr, partner, cid, pooled_ptr


# ---- a. the pair-pool index ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("name", list(ref.index_cases()))
def test_pair_index(dev, name, share):
    from deepmetv2_amd import _native
    ptr, partner, cid_ref, pp_ref = _matching(name, share)
    N, C = len(partner), int(pp_ref[-1])
    pd = torch.from_numpy(partner).to(torch.int32).to(dev)
    ptrd = torch.from_numpy(ptr).to(dev)
    cid, pp = _native.pool_pairs_index(pd, ptrd)
    assert torch.equal(pp.cpu(), torch.from_numpy(pp_ref))
    assert torch.equal(cid.cpu(), torch.from_numpy(cid_ref))
    # the event of every pooled row: the only place a wrong event at a repeated ptr value shows (the events it would
    # skip are empty and add nothing to pooled_ptr)
    x = torch.zeros(N, 1, device=dev)
    mx, arg, mean, pb = _native.pool_pairs(x, pd, cid, ptrd, C, False, False, True)
    assert mx is None and arg is None and mean is None
    pb_ref = ref.pool_pairs(np.zeros((N, 1), np.float32), partner, cid_ref, ptr, C)[3]
    assert torch.equal(pb.cpu(), torch.from_numpy(pb_ref))


# ---- b. pair pooling, forward and backward --------------------------------------------------------------------------------
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("F", [1, 3, 8, 64, 65])
def test_pool_pairs_forward_backward(dev, F, share):
    from deepmetv2_amd import _native
    ptr, partner, cid_ref, pp_ref = _matching("pool", share)
    N, C = len(partner), int(pp_ref[-1])
    rng = np.random.default_rng(100 * F + int(10 * share))
    x = ref.tie_grid(rng, (N, F))
    mx_ref, arg_ref, mean_ref, pb_ref = ref.pool_pairs(x, partner, cid_ref, ptr, C)
    assert 0 in pb_ref and 2 in pb_ref and 3 in pb_ref and 1 not in pb_ref      # never the empty event
    if share < 1.0:
        u = np.flatnonzero(partner > np.arange(N))
        tie = x[u] == x[partner[u]]
        assert tie.any() and np.isnan(mean_ref).any()                  # the inputs do tie, and inf meets -inf
        if F >= 8:
            assert (np.signbit(x[u]) != np.signbit(x[partner[u]]))[tie].any()           # -0.0 against +0.0
    xd = torch.from_numpy(x).to(dev)
    pd = torch.from_numpy(partner).to(torch.int32).to(dev)
    cidd = torch.from_numpy(cid_ref).to(dev)
    ptrd = torch.from_numpy(ptr).to(dev)

    def check(out, want_max, want_mean, want_batch):
        mx, arg, mean, pb = out
        assert (mx is not None) == want_max == (arg is not None)
        assert (mean is not None) == want_mean and (pb is not None) == want_batch
        if want_max:
            assert _same_bits(mx, mx_ref)
            assert torch.equal(arg.cpu(), torch.from_numpy(arg_ref))
        if want_mean:
            assert _same_bits(mean, mean_ref)
        if want_batch:
            assert torch.equal(pb.cpu(), torch.from_numpy(pb_ref))

    check(_native.pool_pairs(xd, pd, cidd, ptrd, C, True, True, True), True, True, True)
    for p in (ptrd, None):
        check(_native.pool_pairs(xd, pd, cidd, p, C, True, False, False), True, False, False)
        check(_native.pool_pairs(xd, pd, cidd, p, C, False, True, False), False, True, False)
    check(_native.pool_pairs(xd, pd, cidd, ptrd, C, False, False, True), False, False, True)
    with pytest.raises(RuntimeError, match="pooled_batch needs B > 0"):            # refused on the host, no launch
        _native.pool_pairs(xd, pd, cidd, None, C, False, False, True)

    # backward: quarter-valued gradients, so g_max + g_mean / 2 is exact whatever way it is evaluated
    g_max = (rng.integers(-8, 9, (C, F)) * 0.25).astype(np.float32)
    g_mean = (rng.integers(-8, 9, (C, F)) * 0.25 + 0.125).astype(np.float32)
    argd = torch.from_numpy(arg_ref).to(dev)
    for gm, ga in ((g_max, None), (None, g_mean), (g_max, g_mean)):
        want = ref.pool_pairs_bwd(gm, arg_ref if gm is not None else None, ga, partner, cid_ref, F)
        got = _native.pool_pairs_bwd(torch.from_numpy(gm).to(dev) if gm is not None else None,
                                     argd if gm is not None else None,
                                     torch.from_numpy(ga).to(dev) if ga is not None else None, pd, cidd, F, C)
        assert _same_bits(got, want), (gm is not None, ga is not None)


# ---- c. the public pooling functions past one chunk, with an interior and a trailing empty event ------------------------
PUBLIC_SIZES = [257, 0, 513, 1, 0]


@pytest.fixture(scope="module")
def public_case(dev):
    import deepmetv2_amd as dm
    B = len(PUBLIC_SIZES)
    x, batch, ptr = _ragged(PUBLIC_SIZES, 8, seed=21)
    xd = (torch.round(x * 2) / 2).to(dev)                     # halves: many ties inside a pair
    bd = batch.to(dev)
    dm.register_batch(bd, ptr.to(dev), B)
    ei = dm.to_undirected(dm.knn_graph(xd, 6, bd, loop=False), num_nodes=xd.shape[0])
    cl = dm.graclus(ei, dm.normalized_cut_2d(ei, xd), xd.shape[0], batch=bd, seed=5)
    c_ref, _p = _ref_graclus(ei, xd.shape[0], ptr, dm.normalized_cut_2d(ei, xd), 5)
    assert torch.equal(cl.cpu(), c_ref)
    return types.SimpleNamespace(xd=xd, bd=bd, ptr=ptr, ei=ei, cl=cl, B=B)


def _pooled_ptr_of(pb_ref, B):
    counts = torch.bincount(pb_ref, minlength=B)
    return counts, torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_public_pool_x_past_one_chunk(dev, public_case, mode):
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import _batch_registry, _registry_get
    c = public_case
    x = c.xd.cpu()
    out_ref, route, inv, pb_ref = _pool_reference(c.cl.cpu(), x, c.bd.cpu(), mode)
    xg = c.xd.clone().requires_grad_(True)
    out, pb = (dm.max_pool_x if mode == "max" else dm.avg_pool_x)(c.cl, xg, c.bd)
    gup = (torch.randint(-8, 9, out.shape, generator=torch.Generator().manual_seed(8)) * 0.25)
    out.backward(gup.to(dev))
    if mode == "max":
        assert torch.equal(out.detach().cpu(), out_ref)
        assert torch.equal(xg.grad.cpu(), torch.where(route, gup[inv], torch.zeros_like(x)))
    else:
        # halves: (x_u + x_v) * 0.5 and g * 0.5 are exact, and so is the reference's sum / count
        assert torch.equal(out.detach().cpu(), out_ref)
        cnt = torch.bincount(inv).to(torch.float32)
        assert torch.equal(xg.grad.cpu(), gup[inv] / cnt[inv].view(-1, 1))
    assert torch.equal(pb.cpu(), pb_ref)
    info = _registry_get(_batch_registry, pb)
    counts, pooled_ptr = _pooled_ptr_of(pb_ref, c.B)
    assert info is not None and info.num_events == c.B
    assert torch.equal(info.ptr.cpu(), pooled_ptr)
    assert info.max_nodes == int(counts.max()) and info.min_nodes == int(counts.min()) == 0


def test_public_max_pool_past_one_chunk(dev, public_case):
    import deepmetv2_amd as dm
    from deepmetv2_amd.data import Batch
    c = public_case
    N = c.xd.shape[0]
    pos = (torch.randint(-8, 9, (N, 3), generator=torch.Generator().manual_seed(2)) * 0.5).to(dev)
    b = Batch(c.xd, torch.zeros(c.B, 1, device=dev), c.bd, c.ptr.to(dev), max(PUBLIC_SIZES), min_nodes=0)
    b.pos, b.edge_index = pos, c.ei
    ob = dm.max_pool(c.cl, b)
    x_ref, _r, inv, pb_ref = _pool_reference(c.cl.cpu(), c.xd.cpu(), c.bd.cpu(), "max")
    pos_ref, _r2, _i2, _pb2 = _pool_reference(c.cl.cpu(), pos.cpu(), c.bd.cpu(), "mean")
    assert torch.equal(ob.x.cpu(), x_ref) and torch.equal(ob.batch.cpu(), pb_ref)
    assert torch.equal(ob.pos.cpu(), pos_ref)                  # halves: the mean of two is exact
    edges = {(int(inv[a]), int(inv[b_])) for a, b_ in c.ei.cpu().t().tolist() if inv[a] != inv[b_]}
    assert ob.edge_index.cpu().t().tolist() == [list(k) for k in sorted(edges)]
    counts, pooled_ptr = _pooled_ptr_of(pb_ref, c.B)
    assert torch.equal(ob.ptr.cpu(), pooled_ptr) and ob.num_graphs == c.B
    assert ob.max_nodes == int(counts.max()) and ob.min_nodes == int(counts.min()) == 0


# ---- d. graclus ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_graclus_directed_rows(dev, weighted):
    import deepmetv2_amd as dm
    sizes = [1, 2, 17, 500, 1500]
    x, batch, ptr = _ragged(sizes, 3, seed=31)
    xd, bd = x.to(dev), batch.to(dev)
    ei = dm.knn_graph(xd, 6, bd, loop=False)                  # row u lists who u points at; nothing points back by rule
    N = xd.shape[0]
    pairs = set(zip(*ei.cpu().tolist()))
    assert any((b, a) not in pairs for a, b in pairs)        # the graph is directed
    w = dm.normalized_cut_2d(ei, xd) if weighted else None
    for mr in (0, 1, 2):
        cl = dm.graclus(ei, w, N, batch=bd, seed=13, max_rounds=mr)
        c_ref, p_ref = _ref_graclus(ei, N, ptr, w, 13, mr)
        assert torch.equal(cl.cpu(), c_ref), mr
        assert torch.equal(_partner(cl).cpu().long(), p_ref), mr


def _csr_with_entries_to_ignore(sizes, seed):
    """A CSR whose rows mix valid neighbours with -1, N, N + 5 and nodes of the other events, every row ascending; some
    rows hold nothing else.  Also the same graph with those entries deleted."""
    rng = np.random.default_rng(seed)
    ptr = ref.ptr_of(sizes)
    N = int(ptr[-1])
    rows, clean, keep = [], [], []
    for b, n in enumerate(sizes):
        lo = int(ptr[b])
        others = np.concatenate([np.arange(0, lo), np.arange(lo + n, N)])
        for i in range(n):
            kind = rng.integers(0, 4)              # 0: only entries to ignore, 3: only valid neighbours, else both
            valid = lo + rng.choice(n, size=min(n, int(rng.integers(1, 5))), replace=False) if kind else np.zeros(0, int)
            junk = np.concatenate([rng.choice([-1, N, N + 5], size=int(rng.integers(1, 4))),
                                   rng.choice(others, size=int(rng.integers(0, 3)))]) if kind != 3 else np.zeros(0, int)
            entries = np.sort(np.concatenate([valid, junk]).astype(np.int64), kind="stable")
            inside = (entries >= lo) & (entries < lo + n)
            rows.append(entries)
            clean.append(entries[inside])
            keep.append(inside)
    csr = []
    for rr in (rows, clean):
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
        csr.append((rowptr, np.concatenate(rr).astype(np.int64)))
    return ptr, csr[0], csr[1], np.concatenate(keep)


@pytest.mark.parametrize("weighted", [False, True])
def test_graclus_ignores_edges_out_of_block_and_out_of_range(dev, weighted):
    from deepmetv2_amd import _native
    ptr, (rowptr, col), (rowptr_c, col_c), keep = _csr_with_entries_to_ignore([40, 1, 25], seed=3)
    N = int(ptr[-1])
    assert (col == -1).any() and (col == N).any() and (col == N + 5).any() and len(col_c) < len(col)
    assert np.array_equal(col[keep], col_c)
    only_junk = [u for u in range(N) if rowptr[u + 1] > rowptr[u] and rowptr_c[u + 1] == rowptr_c[u]]
    assert len(only_junk) >= 3
    w = (np.random.default_rng(4).integers(0, 4, len(col)) * 0.25).astype(np.float32) if weighted else None
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    ptrd = t(ptr, torch.int64)
    for mr in (0, 1):
        c_ref, p_ref, _r = ref.graclus(rowptr, col, w, ptr, 9, mr)
        cl, pa, _ = _native.graclus(t(rowptr, torch.int64), t(col, torch.int32), None if w is None else t(w, torch.float32),
                                    ptrd, 9, mr)
        assert torch.equal(cl.cpu(), torch.from_numpy(c_ref)) and torch.equal(pa.cpu().long(), torch.from_numpy(p_ref))
        cl2, pa2, _ = _native.graclus(t(rowptr_c, torch.int64), t(col_c, torch.int32),
                                      None if w is None else t(w[keep], torch.float32), ptrd, 9, mr)
        assert torch.equal(cl2, cl) and torch.equal(pa2, pa)
        assert torch.equal(cl.cpu()[only_junk], torch.tensor(only_junk))          # nothing to match with
    assert bool((pa >= 0).any())


@pytest.fixture(scope="module")
def lds_cap_graph(dev):
    import deepmetv2_amd as dm
    sizes = [16384, 16385]                 # DMET_GRACLUS_LDS_NODES and one more: state in LDS, state in the workspace
    xd, bd, ptr, ei = _knn_sym(dev, sizes, 3, 2, seed=9)          # about 4 neighbours per node
    return xd, bd, ptr, ei, dm.normalized_cut_2d(ei, xd)


@pytest.mark.parametrize("max_rounds", [0, 1])
def test_graclus_at_the_lds_cap(dev, lds_cap_graph, max_rounds):
    import deepmetv2_amd as dm
    xd, bd, ptr, ei, w = lds_cap_graph
    N = xd.shape[0]
    cl = dm.graclus(ei, w, N, batch=bd, seed=11, max_rounds=max_rounds)
    c_ref, p_ref = _ref_graclus(ei, N, ptr, w, 11, max_rounds)
    assert torch.equal(cl.cpu(), c_ref)
    assert torch.equal(_partner(cl).cpu().long(), p_ref)
    assert int((p_ref[:16384] >= 0).sum()) > 8192 and int((p_ref[16384:] >= 0).sum()) > 8192


@pytest.mark.parametrize("weighted", [False, True])
def test_graclus_many_tiny_and_empty_blocks(dev, weighted):
    import deepmetv2_amd as dm
    rng = np.random.default_rng(6)
    sizes = rng.integers(0, 9, 700)
    sizes[[0, 350, 699]] = 0
    ptr = ref.ptr_of(sizes)
    N = int(ptr[-1])
    rows, cols = [], []
    for lo, n in zip(ptr[:-1], sizes):
        for _ in range(int(n) * 3 // 2):                      # random pairs inside the event, both directions
            i, j = rng.integers(0, n, 2)
            rows += [lo + i, lo + j]
            cols += [lo + j, lo + i]
    ei_np = np.array([rows, cols], dtype=np.int64)
    ei = torch.from_numpy(ei_np).to(dev)
    w_np = (rng.integers(0, 4, ei_np.shape[1]) * 0.25).astype(np.float32) if weighted else None
    w = None if w_np is None else torch.from_numpy(w_np).to(dev)
    bd = torch.repeat_interleave(torch.arange(700), torch.from_numpy(sizes)).to(dev)
    dm.register_batch(bd, torch.from_numpy(ptr).to(dev), 700)
    rowptr, col, ws = ref.to_csr(ei_np, N, w_np)
    c_ref, p_ref, _r = ref.graclus(rowptr, col, ws, ptr, 17)
    cl = dm.graclus(ei, w, N, batch=bd, seed=17)
    assert torch.equal(cl.cpu(), torch.from_numpy(c_ref))
    assert torch.equal(_partner(cl).cpu().long(), torch.from_numpy(p_ref))
    one = dm.graclus(ei, w, N, seed=17)                        # no events known: ptr = [0, N], one block
    assert torch.equal(one, cl) and torch.equal(_partner(one), _partner(cl))
    c_one, p_one, _r = ref.graclus(rowptr, col, ws, np.array([0, N]), 17)
    assert np.array_equal(c_one, c_ref) and np.array_equal(p_one, p_ref)


@pytest.mark.parametrize("kind", ["four_levels", "signed", "infinite"])
def test_graclus_tied_negative_and_infinite_weights(dev, kind):
    import deepmetv2_amd as dm
    xd, bd, ptr, ei = _radius_graph_loops_duplicates(dev)
    N, E = xd.shape[0], ei.shape[1]
    g = torch.Generator().manual_seed(3)
    if kind == "four_levels":
        w = torch.randint(0, 4, (E,), generator=g) * 0.25
    elif kind == "signed":
        w = torch.rand(E, generator=g) * 2 - 1
        assert bool((w < 0).any())
    else:
        w = torch.rand(E, generator=g)
        r = torch.rand(E, generator=g)
        w[r < 0.01] = float("inf")
        w[r > 0.99] = float("-inf")
        assert bool(w.isposinf().any()) and bool(w.isneginf().any())
    wd = w.to(dev)
    for mr in (0, 1):
        cl = dm.graclus(ei, wd, N, batch=bd, seed=3, max_rounds=mr)
        c_ref, p_ref = _ref_graclus(ei, N, ptr, wd, 3, mr)
        assert torch.equal(cl.cpu(), c_ref), mr
        assert torch.equal(_partner(cl).cpu().long(), p_ref), mr


# ---- e. the normalized cut ------------------------------------------------------------------------------------------------
def _cut_edges(E, N, rng):
    """Unsorted edges with duplicates and self loops; the last 8 nodes appear in row only (in-degree 0); from E = 255
    on some endpoints are -1 and N."""
    row = rng.integers(0, N, E)
    col = rng.integers(0, N - 8, E)
    if E >= 255:
        row[0:6] = [N - 1, N - 1, 3, 3, 5, N - 2]
        col[0:6] = [0, 0, 3, 3, 5, 1]                          # duplicates, self loops, rows of in-degree 0
        row[[10, 100, E - 1]] = [-1, N, 2]
        col[[20, 100, E - 1, E - 2]] = [N, -1, N, -1]
    return row, col


@pytest.mark.parametrize("E", [1, 255, 256, 257, 5000])
def test_normalized_cut_exact(dev, E):
    import deepmetv2_amd as dm
    N = 48
    rng = np.random.default_rng(E)
    row, col = _cut_edges(E, N, rng)
    ei = torch.from_numpy(np.stack([row, col])).to(dev)
    attr = (rng.integers(0, 513, E) / 256.0).astype(np.float32)         # multiples of 2^-8
    if E >= 255:
        attr[:2], attr[5] = 0.0, 1.0                                   # 0 * (inf + 1/deg) = NaN; 1 * (inf + 1/deg) = inf
    want = ref.normalized_cut(row, col, N, attr=attr)
    got = dm.normalized_cut(ei, torch.from_numpy(attr).to(dev), N)
    assert _same_bits(got, torch.from_numpy(want))
    if E >= 255:
        bad = (row < 0) | (row >= N) | (col < 0) | (col >= N)
        assert bad.sum() >= 5 and np.isnan(want[bad]).all() and np.isnan(want[:2]).all()
        assert np.isinf(want[5]) and np.isfinite(want[~bad & (row < N - 8)]).all()
    for D, q in [(D, q) for D in (1, 2, 3, 64) for q in (16, 1024)]:
        # multiples of 2^-4 in [-4, 4]: every square and every partial sum is exact in double, and in float32 too.
        # Multiples of 2^-10: squares of up to 28 bits and sums of up to 34, still exact in double, but no longer in
        # float32, so this grid also tells a float32 accumulation from the header's double one.
        x = (rng.integers(-4 * q, 4 * q + 1, (N, D)) / float(q)).astype(np.float32)
        x[N - 1] = x[0]                                                # distance 0 from a node of in-degree 0: NaN
        want = ref.normalized_cut(row, col, N, x=x)
        got = dm.normalized_cut_2d(ei, torch.from_numpy(x).to(dev))
        assert _same_bits(got, torch.from_numpy(want)), (D, q)
        if E >= 255:
            assert np.isnan(want[:2]).all() and np.isnan(want[bad]).all()


@pytest.mark.parametrize("D", [2, 64])
def test_normalized_cut_general(dev, D):
    """Gaussian coordinates against a float64 evaluation of the same formula.  The kernel rounds four times in float32
    (the norm, 1/deg of one endpoint counted once in the sum, the sum, the product), each at most 2^-24 relative, on top
    of a correctly rounded double square root: 4 * 2^-24 = 2.4e-7 < 3e-7."""
    import deepmetv2_amd as dm
    N, E = 300, 5000
    rng = np.random.default_rng(D)
    row = rng.integers(0, N, E)
    col = np.concatenate([rng.integers(0, N, E - N), rng.permutation(N)])       # every node has an in-degree
    x = rng.standard_normal((N, D)).astype(np.float32)
    got = dm.normalized_cut_2d(torch.from_numpy(np.stack([row, col])).to(dev), torch.from_numpy(x).to(dev))
    x64 = x.astype(np.float64)
    deg = np.bincount(col, minlength=N).astype(np.float64)
    w64 = np.sqrt(((x64[row] - x64[col]) ** 2).sum(1)) * (1.0 / deg[row] + 1.0 / deg[col])
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(w64), rtol=3e-7, atol=0)
    attr = rng.random(E).astype(np.float32)
    got = dm.normalized_cut(torch.from_numpy(np.stack([row, col])).to(dev), torch.from_numpy(attr).to(dev), N)
    a64 = attr.astype(np.float64) * (1.0 / deg[row] + 1.0 / deg[col])
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(a64), rtol=3e-7, atol=0)

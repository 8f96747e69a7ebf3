"""Graph coarsening without a GPU: the CPU restatement of the graclus contract (tests/pool_reference.py), argument
validation of the new C entries (include/dmet.h "Graph coarsening"), and the Python-level errors."""
import os
import shutil

import numpy as np
import pytest
import torch

import pool_reference as ref


def _sym_random_graph(sizes, deg, seed):
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows, cols = [], []
    for b, n in enumerate(sizes):
        lo = ptr[b]
        if n < 2:
            continue
        for i in range(n):
            for j in rng.choice(n, size=min(deg, n), replace=False):
                rows += [lo + i, lo + j]
                cols += [lo + j, lo + i]
    return np.array([rows, cols], dtype=np.int64), ptr


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("max_rounds", [0, 1, 2])
def test_reference_matching_is_valid_and_maximal(weighted, max_rounds):
    ei, ptr = _sym_random_graph([1, 2, 17, 60, 0, 130], 4, seed=3 + max_rounds)
    N = int(ptr[-1])
    w = np.random.default_rng(7).random(ei.shape[1]).astype(np.float32) if weighted else None
    rowptr, col, ws = ref.to_csr(ei, N, w)
    cluster, partner, rounds = ref.graclus(rowptr, col, ws, ptr, seed=12345, max_rounds=max_rounds)
    ref.check_matching(cluster, partner, ei, ptr)
    if max_rounds:
        assert rounds.max() <= max_rounds
    leaders = cluster == np.arange(N)
    assert leaders.sum() < N          # something was matched


def test_reference_finisher_runs_with_one_round():
    """max_rounds=1 leaves nodes unmatched after the parallel round on a dense event: the finisher takes them."""
    ei, ptr = _sym_random_graph([200], 8, seed=1)
    rowptr, col, _ = ref.to_csr(ei, 200)
    c1, p1, r1 = ref.graclus(rowptr, col, None, ptr, seed=5, max_rounds=1)
    c0, p0, r0 = ref.graclus(rowptr, col, None, ptr, seed=5)
    assert r1[0] == 1 and r0[0] > 1
    ref.check_matching(c1, p1, ei, ptr)
    assert not np.array_equal(c1, c0)


def test_reference_colour_function_and_tie_rule():
    assert ref.lowbias32(0) == 0
    assert ref._best([4, 2, 9], [1.0, 1.0, 1.0]) == 4             # all equal: the first candidate
    assert ref._best([4, 2, 9], [1.0, 3.0, 3.0]) == 2             # strictly greater only
    assert ref._best([4, 2], [float("nan"), 5.0]) == 4            # IEEE compare: nothing beats a leading NaN
    assert ref._best([4, 2, 9], None) == 4
    # both colours occur, and they change between rounds
    s = 99
    k0, k1 = ref.lowbias32(s), ref.lowbias32((s + 0x9E3779B9) & ref.M32)
    c0 = [ref.is_red(u, k0) for u in range(256)]
    c1 = [ref.is_red(u, k1) for u in range(256)]
    assert 64 < sum(c0) < 192 and c0 != c1


def test_reference_self_loops_and_duplicates_are_harmless():
    ei, ptr = _sym_random_graph([40], 3, seed=4)
    loops = np.stack([np.arange(40), np.arange(40)])
    ei2 = np.concatenate([ei, loops, ei[:, :10]], axis=1)
    a = ref.graclus(*ref.to_csr(ei, 40)[:2], None, ptr, seed=8)
    b = ref.graclus(*ref.to_csr(ei2, 40)[:2], None, ptr, seed=8)
    assert np.array_equal(a[0], b[0])


# ---- the C entries: argument validation through ctypes, no GPU ---------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def test_graclus_argument_validation(lib):
    assert lib.dmet_graclus_workspace_bytes(1000) == 8000
    rc = lib.dmet_graclus_f32(None, None, None, None, 1, -1, 0, 0, None, None, None, None, 0, None)
    assert rc == -22 and b"bad sizes" in lib.dmet_last_error()
    rc = lib.dmet_graclus_f32(None, None, None, None, 1, 10, 0, -1, None, None, None, None, 0, None)
    assert rc == -22 and b"max_rounds=-1" in lib.dmet_last_error()
    rc = lib.dmet_graclus_f32(None, None, None, None, 1, 10, 0, 0, None, None, None, None, 0, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_graclus_f32(None, None, None, None, 0, 0, 7, 0, None, None, None, None, 0, None) == 0


def test_normalized_cut_argument_validation(lib):
    assert lib.dmet_normalized_cut_workspace_bytes(10) == 40
    rc = lib.dmet_normalized_cut_2d_f32(None, None, 10, 10, None, 65, None, None, 0, None)
    assert rc == -22 and b"D=65" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_2d_f32(None, None, 10, 10, None, 0, None, None, 0, None)
    assert rc == -22 and b"D=0" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_f32(None, None, -1, 10, None, None, None, 0, None)
    assert rc == -22 and b"bad sizes" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_f32(None, None, 5, 0, None, None, None, 0, None)
    assert rc == -22 and b"N=0" in lib.dmet_last_error()
    rc = lib.dmet_normalized_cut_f32(None, None, 5, 5, None, None, None, 0, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_normalized_cut_f32(None, None, 0, 0, None, None, None, 0, None) == 0
    assert lib.dmet_normalized_cut_2d_f32(None, None, 0, 5, None, 64, None, None, 0, None) == 0


def test_pool_pairs_argument_validation(lib):
    assert lib.dmet_pool_pairs_workspace_bytes(100, 4) == 416
    rc = lib.dmet_pool_pairs_index(None, None, 1, -1, None, None, None, 0, None)
    assert rc == -22 and b"bad sizes" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_index(None, None, 0, 5, None, None, None, 0, None)
    assert rc == -22 and b"B=0" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_index(None, None, 2, 5, None, None, None, 0, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_pool_pairs_index(None, None, 0, 0, None, None, None, 0, None) == 0
    rc = lib.dmet_pool_pairs_f32(None, 10, 0, None, None, None, 1, 5, None, None, None, None, None)
    assert rc == -22 and b"F=0" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_f32(None, 10, 4, None, None, None, 1, 11, None, None, None, None, None)
    assert rc == -22 and b"C=11" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_f32(None, 10, 4, None, None, None, 1, 5, None, None, None, None, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_pool_pairs_f32(None, 0, 4, None, None, None, 1, 0, None, None, None, None, None) == 0
    rc = lib.dmet_pool_pairs_bwd_f32(None, None, None, None, None, 10, 4, 11, None, None)
    assert rc == -22 and b"C=11" in lib.dmet_last_error()
    rc = lib.dmet_pool_pairs_bwd_f32(None, None, None, None, None, 10, 4, 5, None, None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    assert lib.dmet_pool_pairs_bwd_f32(None, None, None, None, None, 0, 4, 0, None, None) == 0


# ---- Python-level errors ---------------------------------------------------------------------------------------------
def test_python_errors_without_a_gpu():
    import deepmetv2_amd as dm
    ei = torch.tensor([[0, 1], [1, 0]])
    x = torch.randn(2, 3)
    cl = torch.tensor([0, 0])
    b = torch.zeros(2, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        dm.max_pool_x(cl, x, b, size=4)
    with pytest.raises(NotImplementedError):
        dm.avg_pool_x(cl, x, b, batch_size=1, size=4)
    for call in (lambda: dm.graclus(ei), lambda: dm.normalized_cut(ei, torch.ones(2)),
                 lambda: dm.normalized_cut_2d(ei, x), lambda: dm.max_pool_x(cl, x, b), lambda: dm.avg_pool_x(cl, x, b),
                 lambda: dm.global_max_pool(x, b), lambda: dm.global_mean_pool(x, None),
                 lambda: dm.global_add_pool(x, b)):
        with pytest.raises(RuntimeError, match="non-GPU tensor"):
            call()


# ---- the references of the pair-pool index, pair pooling and the normalized cut, each against a brute force ------------
POOL_SIZES = [257, 0, 513, 1]            # the events tests/test_gpu_pool_edges.py pools
SHARES = [0.0, 0.3, 1.0]


def _check_valid_matching(partner, ptr):
    N = len(partner)
    ev = ref.event_of(ptr, np.arange(N))
    for u in range(N):
        v = int(partner[u])
        if v < 0:
            assert v == -1
            continue
        assert v != u and 0 <= v < N and partner[v] == u and ev[u] == ev[v]


@pytest.mark.parametrize("share", SHARES)
def test_random_matching_is_valid_and_straddles_chunks(share):
    cases = dict(ref.index_cases(), pool=POOL_SIZES, small=[3, 0, 8, 1, 2])
    for name, sizes in cases.items():
        ptr = ref.ptr_of(sizes)
        partner = ref.random_matching(ptr, np.random.default_rng(5), share)
        assert partner.dtype == np.int64 and len(partner) == ptr[-1]
        _check_valid_matching(partner, ptr)
        paired = int((partner >= 0).sum())
        if share == 1.0:
            assert paired == 0
            continue
        if share == 0.0:
            assert paired == sum(n - n % 2 for n in sizes)              # every event: all but an odd one out
        else:
            assert 0 < paired < sum(n - n % 2 for n in sizes)
        if max(sizes) > 256:
            u = np.flatnonzero(partner >= 0)
            lo = ptr[ref.event_of(ptr, u)]
            assert bool((((u - lo) // 256) != ((partner[u] - lo) // 256)).any()), name


def _pair_index_brute(partner, ptr):
    clusters = {}
    for u, p in enumerate(partner.tolist()):
        clusters.setdefault(min(u, p) if p >= 0 else u, []).append(u)
    cid = [0] * len(partner)
    for c, lead in enumerate(sorted(clusters)):
        for u in clusters[lead]:
            cid[u] = c
    pooled_ptr = [0]
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        pooled_ptr.append(pooled_ptr[-1] + sum(1 for lead in clusters if lo <= lead < hi))
    return np.array(cid, np.int64), np.array(pooled_ptr, np.int64)


@pytest.mark.parametrize("share", SHARES)
def test_pair_index_reference_vs_cluster_dict(share):
    for sizes in ([3, 0, 8, 1, 2], [0, 0, 5], [7, 0, 0], [1], [40, 9, 0, 60], POOL_SIZES):
        ptr = ref.ptr_of(sizes)
        partner = ref.random_matching(ptr, np.random.default_rng(len(sizes)), share)
        cid, pp = ref.pair_index(partner, ptr)
        cid_b, pp_b = _pair_index_brute(partner, ptr)
        assert np.array_equal(cid, cid_b) and np.array_equal(pp, pp_b)
        assert cid.dtype == np.int64 and pp.dtype == np.int64
    # a partner that is no valid lower index leaves the node a leader
    cid, pp = ref.pair_index(np.array([-1, 5, -7, 2]), np.array([0, 4]))
    assert cid.tolist() == [0, 1, 2, 2] and pp.tolist() == [0, 3]


def _index_as_the_kernels_walk(partner, ptr, rank_restarts=False, scan_carry_dropped=False, first_event=False):
    """(cid, pooled_ptr, pooled_batch) computed the way csrc/pool.hip is organised -- events walked in chunks of 256
    nodes with a carried rank, counts scanned in chunks of 256 events with a carried base, the event of a leader found by
    bisection over ptr -- with a switch for each plausible slip."""
    ptr = np.asarray(ptr, np.int64)
    N, B = len(partner), len(ptr) - 1
    lead = ref.leaders(partner)
    is_lead = lead == np.arange(N)
    rank = np.zeros(N, np.int64)
    cnt = np.zeros(B, np.int64)
    for b in range(B):
        base = 0
        for c0 in range(int(ptr[b]), int(ptr[b + 1]), 256):
            f = is_lead[c0:min(c0 + 256, int(ptr[b + 1]))]
            rank[c0:c0 + len(f)] = (0 if rank_restarts else base) + np.cumsum(f) - f
            base += int(f.sum())
        cnt[b] = base
    pooled_ptr = np.zeros(B + 1, np.int64)
    base = 0
    for c0 in range(0, B, 256):
        part = np.cumsum(cnt[c0:c0 + 256])
        pooled_ptr[c0 + 1:c0 + 1 + len(part)] = (0 if scan_carry_dropped else base) + part
        base += int(part[-1])
    ev = np.searchsorted(ptr[:B], np.arange(N), side="right") - 1
    if first_event:
        ev = np.searchsorted(ptr[:B], ptr[ev], side="left")
    cid = pooled_ptr[ev[lead]] + rank[lead]
    C = int(is_lead.sum())
    pooled_batch = np.full(C, -1, np.int64)
    ok = is_lead & (cid >= 0) & (cid < C)
    pooled_batch[cid[ok]] = ev[ok]
    return cid, pooled_ptr, pooled_batch


def _index_with_batch(partner, ptr):
    cid, pp = ref.pair_index(partner, ptr)
    u = np.flatnonzero(ref.leaders(partner) == np.arange(len(partner)))
    pb = np.zeros(int(pp[-1]), np.int64)
    pb[cid[u]] = ref.event_of(ptr, u)
    return cid, pp, pb


@pytest.mark.parametrize("share", SHARES)
def test_gpu_index_inputs_tell_wrong_kernels_from_right(share):
    """Every input of tests/test_gpu_pool_edges.py's index and pooling tests, against three wrong index kernels.
    A find_event that returns the FIRST event at a repeated ptr value leaves cid and pooled_ptr as they are (the events
    it skips are empty, so they add nothing to the prefix sum): only pooled_batch shows it, which is why the GPU tests
    check pooled_batch on every one of these inputs."""
    cases = dict(ref.index_cases(), pool=POOL_SIZES)
    caught = {"rank_restarts": set(), "scan_carry_dropped": set(), "first_event": set()}
    for name, sizes in cases.items():
        ptr = ref.ptr_of(sizes)
        partner = ref.random_matching(ptr, np.random.default_rng(11), share)
        want = _index_with_batch(partner, ptr)
        right = _index_as_the_kernels_walk(partner, ptr)
        assert all(np.array_equal(a, b) for a, b in zip(right, want)), name
        for slip in caught:
            got = _index_as_the_kernels_walk(partner, ptr, **{slip: True})
            if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                caught[slip].add(name)
            elif not np.array_equal(got[2], want[2]):
                caught[slip].add(name + ":batch")
    assert caught["rank_restarts"] == {"chunk_edges", "one_event", "scan_carry", "pool"}
    assert caught["scan_carry_dropped"] == {"events_257", "scan_carry"}
    assert caught["first_event"] == {n + ":batch" for n in cases if n != "one_event"}


def _f32(v):
    return np.float32(v)


def _pool_pairs_brute(x, partner, cid, ptr, C):
    N, F = x.shape
    mx, arg = np.zeros((C, F), np.float32), np.zeros((C, F), np.int32)
    mean, pb = np.zeros((C, F), np.float32), np.zeros(C, np.int64)
    for u in range(N):
        v = int(partner[u])
        if 0 <= v < u:
            continue
        c = int(cid[u])
        pb[c] = max(b for b in range(len(ptr) - 1) if ptr[b] <= u)
        for f in range(F):
            xu = _f32(x[u, f])
            if v < 0:
                mx[c, f], arg[c, f], mean[c, f] = xu, u, xu
                continue
            xv = _f32(x[v, f])
            win = bool(xv > xu)
            mx[c, f], arg[c, f] = (xv, v) if win else (xu, u)
            with np.errstate(invalid="ignore"):
                mean[c, f] = _f32(_f32(xu + xv) * _f32(0.5))
    return mx, arg, mean, pb


def _same_bits(a, b):
    """Bit equality of two float32 arrays; NaNs match each other whatever their payload or sign."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("F", [1, 3])
def test_pool_pairs_reference_vs_pair_loop(share, F):
    rng = np.random.default_rng(17 + F)
    ptr = ref.ptr_of([9, 0, 30, 1, 0])
    partner = ref.random_matching(ptr, rng, share)
    N = len(partner)
    cid, pp = ref.pair_index(partner, ptr)
    C = int(pp[-1])
    x = ref.tie_grid(rng, (N, F))
    got = ref.pool_pairs(x, partner, cid, ptr, C)
    want = _pool_pairs_brute(x, partner, cid, ptr, C)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert _same_bits(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[3].dtype == np.int64
    # backward, per (node, channel), in the header's order
    g_max = (rng.integers(-8, 9, (C, F)) * 0.25).astype(np.float32)
    g_mean = (rng.integers(-8, 9, (C, F)) * 0.25 + 0.125).astype(np.float32)
    for gm, ga in ((g_max, None), (None, g_mean), (g_max, g_mean)):
        gx = ref.pool_pairs_bwd(gm, got[1] if gm is not None else None, ga, partner, cid, F)
        for u in range(N):
            for f in range(F):
                c = cid[u]
                g = _f32(gm[c, f]) if gm is not None and got[1][c, f] == u else _f32(0)
                if ga is not None:
                    g = _f32(g + _f32(ga[c, f] * _f32(0.5 if partner[u] >= 0 else 1.0)))
                assert gx[u, f].view(np.int32) == g.view(np.int32), (u, f)


def test_pool_pairs_reference_tie_and_signed_zero_rules():
    x = np.array([[-0.0, 0.0, 1.0, np.inf, -np.inf, 2.0],
                  [0.0, -0.0, 1.0, -np.inf, -np.inf, np.inf]], np.float32)
    partner, ptr = np.array([1, 0]), np.array([0, 2])
    cid, pp = ref.pair_index(partner, ptr)
    mx, arg, mean, pb = ref.pool_pairs(x, partner, cid, ptr, 1)
    assert arg[0].tolist() == [0, 0, 0, 0, 0, 1]                      # only a strictly greater partner wins
    assert _same_bits(mx[0], np.array([-0.0, 0.0, 1.0, np.inf, -np.inf, np.inf], np.float32))
    assert np.signbit(mx[0, 0]) and not np.signbit(mx[0, 1])
    assert np.isnan(mean[0, 3]) and mean[0, 4] == -np.inf and mean[0, 5] == np.inf and pb.tolist() == [0]


def _cut_brute(row, col, N, attr, x):
    """torch.bincount for the degrees, float64 arithmetic for the norm, the float32 steps edge by edge."""
    row_t, col_t = torch.as_tensor(row), torch.as_tensor(col)
    col_ok = (col_t >= 0) & (col_t < N)
    deg = torch.bincount(col_t[col_ok], minlength=N).tolist()
    out = np.zeros(len(row), np.float32)
    for e, (r, c) in enumerate(zip(row.tolist(), col.tolist())):
        if not (0 <= r < N and 0 <= c < N):
            out[e] = np.nan
            continue
        if x is not None:
            acc = 0.0
            for d in range(x.shape[1]):
                t = float(x[r, d]) - float(x[c, d])
                acc += t * t
            a = _f32(acc ** 0.5)
        else:
            a = _f32(attr[e])
        with np.errstate(divide="ignore", invalid="ignore"):
            ir, ic = _f32(1.0) / _f32(deg[r]), _f32(1.0) / _f32(deg[c])
            out[e] = a * _f32(ir + ic)
    return out


@pytest.mark.parametrize("D", [1, 3, 64])
def test_normalized_cut_reference_vs_edge_loop(D):
    rng = np.random.default_rng(D)
    N, E = 23, 120
    row, col = rng.integers(0, N - 4, E), rng.integers(0, N - 8, E)     # nodes 15..18 in row only: in-degree 0
    row[[3, 50]], col[[7, 50, 90]] = [-1, N], [N, -1, N + 3]             # out of range
    x = rng.standard_normal((N, D)).astype(np.float32)
    attr = rng.random(E).astype(np.float32)
    attr[:10] = 0.0
    for a, xx in ((attr, None), (None, x)):
        got = ref.normalized_cut(row, col, N, attr=a, x=xx)
        want = _cut_brute(row, col, N, a, xx)
        assert got.dtype == np.float32 and _same_bits(got, want)
        bad = (row < 0) | (row >= N) | (col < 0) | (col >= N)
        assert np.isnan(got[bad]).all()
        lone = ~bad & (row >= N - 8)
        assert lone.any() and (np.isinf(got[lone]) | (np.isnan(got[lone]) & (a is not None))).all()
    # float64 evaluation of the same formula: four float32 roundings on top of a correctly rounded square root
    ok = ~bad & (row < N - 8)
    deg = np.bincount(col[(col >= 0) & (col < N)], minlength=N).astype(np.float64)   # whatever the edge's row is
    dist = np.sqrt(((x[row[ok]].astype(np.float64) - x[col[ok]].astype(np.float64)) ** 2).sum(1))
    w64 = dist * (1.0 / deg[row[ok]] + 1.0 / deg[col[ok]])
    np.testing.assert_allclose(ref.normalized_cut(row, col, N, x=x)[ok].astype(np.float64), w64, rtol=3e-7, atol=0)

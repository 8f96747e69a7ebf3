"""What the one-workgroup-per-event kernels do with a `ptr` that does not cover the nodes (include/dmet.h, "Nodes no event
owns ..."): topk_kernel, voxel_coarsen_kernel / voxel_write_kernel, edge_match_kernel, components_kernel and
condense_kernel, through their _native wrappers.

One batch serves all five: N = 200 nodes, 13 in front that no event owns, events of 70, 0, 1 and 109 nodes, 7 behind that
no event owns.  The nodes no event owns hold each entry point's stated fill; the owned part equals the reference where the
reference takes a general ptr (select_reference.topk, components_reference.cc_loops, edge_pool_reference's two matchings),
else the same call on the slice [13, 193) with ptr - 13 -- the form the other GPU tests hold to their references -- with
the global ids it returns moved by 13.  A second batch holds a ptr that needs the clamp, [-5, 80, 80, 300], to the bits
of [0, 80, 80, 200].  Scores in {-1, 0, 1} or a permutation, coordinates on the k / 8 lattice, beta in sixteenths: fp32
cannot matter, everything is an integer, equality throughout."""
import numpy as np
import pytest
import torch

import components_reference as cr
import condense_reference as cdr
import edge_pool_reference as er
import select_reference as sr
import voxel_reference as vr

pytestmark = pytest.mark.gpu

N, HEAD, TAIL = 200, 13, 7
SIZES = [70, 0, 1, 109]
LO, HI = HEAD, N - TAIL
PTR = HEAD + cr.ptr_of(SIZES)                                   # [13, 83, 83, 84, 193]
EMPTY = 1                                                       # the event without a node
CLAMP_RAW, CLAMP_SIZES = np.array([-5, 80, 80, 300], dtype=np.int64), [80, 0, 120]
LIMITS = (0, 1)                                                 # lds_nodes: every event in LDS | all but the one-node event
assert PTR.tolist() == [13, 83, 83, 84, 193] and HI - LO == sum(SIZES) and sum(CLAMP_SIZES) == N


@pytest.fixture(autouse=True)
def _drain():
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()
    yield
    dm.raise_deferred_errors()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(got: torch.Tensor, want) -> bool:
    w = want.cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.asarray(want))
    return got.dtype == w.dtype and got.shape == w.shape and torch.equal(got.cpu(), w)


def _same(runs_a, runs_b) -> bool:
    return len(runs_a) == len(runs_b) and all((a is None and b is None) or _eq(a, b) for a, b in zip(runs_a, runs_b))


def _moved(t: torch.Tensor, by: int = HEAD) -> torch.Tensor:
    """Global node ids of a call on the slice, as the call on the whole batch returns them; -1 stays -1."""
    return torch.where(t >= 0, t + by, t)


def _unowned(t: torch.Tensor) -> torch.Tensor:
    return torch.cat([t[:LO], t[HI:]]).cpu()


def _ids(dtype=torch.int64) -> torch.Tensor:
    return torch.cat([torch.arange(LO), torch.arange(HI, N)]).to(dtype)


def _edges(sizes, first, thin):
    """int64 [2, E] (source, target) in the caller's order: edge_pool_reference's width-3 table over the events `sizes`
    whose first node is `first`, a self entry in every one-node event; thin: about two entries in five dropped, so that rows
    hold 0 .. 3 entries."""
    rng = np.random.default_rng(11)
    src, tgt = er._table_edges(sizes, 3, rng)
    ei = np.array([src, tgt], np.int64).reshape(2, -1)
    if thin:
        ei = ei[:, rng.random(ei.shape[1]) < 0.6]
    ones = [int(lo) for lo, n in zip(cr.ptr_of(sizes), sizes) if n == 1]
    ei = np.concatenate([ei, np.array([ones, ones], np.int64).reshape(2, -1)], axis=1)
    return ei[:, rng.permutation(ei.shape[1])] + first


def _grouped(ei, n, dev):
    """(the by-target list of _native over n nodes, the caller-order id of every grouped position)"""
    rowptr, src, tgt, perm = er.group_by_target(ei, n)
    return dict(rowptr=_t(rowptr, dev), src=_t(src, dev), tgt=_t(tgt, dev)), perm


# ---- _topk --------------------------------------------------------------------------------------------------------------------
def test_topk(dev):
    from deepmetv2_amd import _native
    score = sr.scores("ties", [N])
    out_ptr = sr.ptr_of(sr.slots_of(SIZES, 0.5))
    M = int(out_ptr[-1])
    perm, node_map = _native._topk(score.to(dev), _t(PTR, dev), out_ptr.to(dev), M)
    want_perm, want_map = sr.topk(score, torch.from_numpy(PTR), out_ptr, M)
    assert _eq(_unowned(node_map), torch.full((HEAD + TAIL,), -1, dtype=torch.int32))
    assert _eq(perm, want_perm) and _eq(node_map, want_map)
    assert int((want_perm < 0).sum()) == 0 and int((want_map[LO:HI] >= 0).sum()) == M


def test_topk_clamps_ptr(dev):
    from deepmetv2_amd import _native
    score = sr.scores("ties", [N]).to(dev)
    out_ptr = sr.ptr_of(sr.slots_of(CLAMP_SIZES, 0.5)).to(dev)
    M = int(out_ptr[-1])
    runs = [_native._topk(score, _t(p, dev), out_ptr, M) for p in (CLAMP_RAW, cr.ptr_of(CLAMP_SIZES))]
    assert _same(*runs) and int((runs[0][1] >= 0).sum()) == M


# ---- _voxel_coarsen -------------------------------------------------------------------------------------------------------------
def _cells():
    """Event-local cell ids of N lattice points in a 3 x 3 x 3 grid: every quotient is exact."""
    _beta, pos = cdr._lattice(np.random.default_rng(3), N, 3, 5)
    cell = vr.grid_cluster_ref(torch.from_numpy(pos), 0.25, start=0.0, end=0.5)
    assert int(cell.max()) < 27
    return cell.to(torch.int32)


def _cut(run):
    """A _voxel_coarsen result with rowptr and batch cut to the C + 1 and C entries that are written."""
    node_map, order, rowptr, batch, out_ptr, record = (t.cpu() for t in run)
    C = int(record[0])
    return node_map, order, rowptr[:C + 1], batch[:C], out_ptr, record


def test_voxel_coarsen(dev):
    from deepmetv2_amd import _native
    cell = _cells()
    node_map, order, rowptr, batch, out_ptr, record = _cut(_native._voxel_coarsen(cell.to(dev), _t(PTR, dev)))
    fill = torch.full((HEAD + TAIL,), -1, dtype=torch.int64)
    assert _eq(_unowned(node_map), fill) and _eq(_unowned(order), fill)
    s_map, s_order, s_rowptr, s_batch, s_ptr, s_record = _cut(_native._voxel_coarsen(cell[LO:HI].to(dev), _t(PTR - HEAD, dev)))
    assert _eq(node_map[LO:HI], s_map) and _eq(order[LO:HI], _moved(s_order))
    assert _eq(rowptr, s_rowptr + HEAD) and _eq(batch, s_batch) and _eq(out_ptr, s_ptr) and _eq(record, s_record)
    # the counts are those of the owned events alone
    per_event = [np.unique(cell[PTR[b]:PTR[b + 1]].numpy()).size for b in range(len(SIZES))]
    assert out_ptr.tolist() == cr.ptr_of(per_event).tolist() and per_event[EMPTY] == 0
    assert record.tolist() == [sum(per_event), max(per_event), min(per_event)]


def test_voxel_coarsen_clamps_ptr(dev):
    from deepmetv2_amd import _native
    cell = _cells().to(dev)
    runs = [_cut(_native._voxel_coarsen(cell, _t(p, dev))) for p in (CLAMP_RAW, cr.ptr_of(CLAMP_SIZES))]
    assert _same(*runs) and int((runs[0][0] < 0).sum()) == 0


# ---- _edge_match ----------------------------------------------------------------------------------------------------------------
def _match_args(sizes, first, n, dev):
    """(the grouped operands of _native._edge_match without ptr, the caller-order (src, tgt, score, ids) of the references)"""
    ei = _edges(sizes, first, thin=False)
    E = ei.shape[1]
    score = np.random.default_rng(12).permutation(E).astype(np.float32)
    g, perm = _grouped(ei, n, dev)
    return (g["rowptr"], g["src"], g["tgt"], _t(perm, dev), _t(score[perm], dev)), (ei[0], ei[1], score, np.arange(E))


def _state(monkeypatch, form):
    if form == "workspace":
        monkeypatch.setenv("DMET_EDGE_MATCH_STATE", "workspace")
    else:
        monkeypatch.delenv("DMET_EDGE_MATCH_STATE", raising=False)


@pytest.mark.parametrize("form", ("lds", "workspace"))
def test_edge_match(dev, monkeypatch, form):
    from deepmetv2_amd import _native
    _state(monkeypatch, form)
    args, caller = _match_args(SIZES, HEAD, N, dev)
    cluster, partner, edge, rounds, flags = _native._edge_match(*args, _t(PTR, dev), want_rounds=True)
    assert _eq(_unowned(cluster), _ids()) and _eq(_unowned(partner), torch.full((HEAD + TAIL,), -1, dtype=torch.int32))
    assert _eq(_unowned(edge), torch.full((HEAD + TAIL,), -1, dtype=torch.int64))
    want = er.sequential_match(*caller, PTR, N)
    assert _eq(cluster, want[0]) and _eq(partner.long(), want[1]) and _eq(edge, want[2])
    _c, _p, _e, want_rounds, want_flags = er.round_match(*caller, PTR, N)
    assert _eq(rounds, want_rounds) and _eq(flags, want_flags)
    assert int(rounds[EMPTY]) == 0 and int(rounds.max()) > 1 and flags.tolist() == [0, 0, 0]
    assert int((partner[LO:HI] >= 0).sum()) > 0


@pytest.mark.parametrize("form", ("lds", "workspace"))
def test_edge_match_clamps_ptr(dev, monkeypatch, form):
    from deepmetv2_amd import _native
    _state(monkeypatch, form)
    args, _caller = _match_args(CLAMP_SIZES, 0, N, dev)
    runs = [_native._edge_match(*args, _t(p, dev), want_rounds=True) for p in (CLAMP_RAW, cr.ptr_of(CLAMP_SIZES))]
    assert _same(*runs) and runs[0][4].tolist() == [0, 0, 0] and int((runs[0][1] >= 0).sum()) > 0


# ---- _components: connected components ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", LIMITS)
def test_connected_components(dev, limit):
    from deepmetv2_amd import _native
    ei = _edges(SIZES, HEAD, thin=True)
    g, perm = _grouped(ei, N, dev)
    rng = np.random.default_rng(13)
    node_keep, edge_keep = rng.random(N) < 0.8, rng.random(ei.shape[1]) < 0.8
    node_keep[[2, N - 3]], node_keep[[3, N - 2]] = False, True      # both values among the nodes no event owns, either side
    for masked in (False, True):
        masks = dict(edge_mask=_t(edge_keep[perm], dev), node_mask=_t(node_keep, dev)) if masked else {}
        labels, core, ncl, flags = _native._components(_t(PTR, dev), N, lds_nodes=limit, **masks, **g)
        assert core is None and ncl is None and flags.tolist() == [0, 0, 0, 0]
        fill = torch.where(torch.from_numpy(node_keep), torch.arange(N), -1) if masked else torch.arange(N)
        assert _eq(_unowned(labels), _unowned(fill))
        want, bad = cr.cc_loops(N, ei[1], ei[0], PTR, edge_keep if masked else None, node_keep if masked else None)
        assert _eq(labels, want) and bad == [0, 0]
        assert int((labels[LO:HI].cpu() != torch.arange(LO, HI)).sum()) > 0


@pytest.mark.parametrize("limit", LIMITS)
def test_connected_components_clamp_ptr(dev, limit):
    from deepmetv2_amd import _native
    g, _perm = _grouped(_edges(CLAMP_SIZES, 0, thin=True), N, dev)
    runs = [_native._components(_t(p, dev), N, lds_nodes=limit, **g) for p in (CLAMP_RAW, cr.ptr_of(CLAMP_SIZES))]
    assert _same(*runs) and runs[0][3].tolist() == [0, 0, 0, 0]


# ---- _components: DBSCAN --------------------------------------------------------------------------------------------------------
def _table(ei, n, first):
    """nbr[n, 4] int32 of the entries, -1 = empty, every row packed to the left and none full; rows before `first`: empty."""
    local = cr.Graph("t", [n - first], ei[1] - first, ei[0] - first).table(4)
    nbr = np.full((n, 4), -1, dtype=np.int32)
    nbr[first:first + local.shape[0]] = np.where(local >= 0, local + first, -1)
    return nbr


@pytest.mark.parametrize("form", ("list", "table"))
@pytest.mark.parametrize("limit", LIMITS)
def test_dbscan(dev, limit, form):
    """min_samples = 3 with the node itself counted: a row of two or three entries makes a core node."""
    from deepmetv2_amd import _native
    ei = _edges(SIZES, HEAD, thin=True)
    if form == "list":
        whole, part = _grouped(ei, N, dev)[0], _grouped(ei - HEAD, HI - LO, dev)[0]
    else:
        whole = dict(nbr=_t(_table(ei, N, HEAD), dev))
        part = dict(nbr=_t(_table(ei - HEAD, HI - LO, 0), dev))
    kw = dict(min_samples=3, count_self=True, lds_nodes=limit)
    labels, core, ncl, flags = _native._components(_t(PTR, dev), N, **kw, **whole)
    assert _eq(_unowned(labels), torch.full((HEAD + TAIL,), -1, dtype=torch.int64))
    assert _eq(_unowned(core), torch.zeros(HEAD + TAIL, dtype=torch.bool))
    s_labels, s_core, s_ncl, s_flags = _native._components(_t(PTR - HEAD, dev), HI - LO, **kw, **part)
    assert _eq(labels[LO:HI], s_labels) and _eq(core[LO:HI], s_core) and _eq(ncl, s_ncl) and _eq(flags, s_flags)
    assert int(ncl[EMPTY]) == 0 and int(ncl.max()) > 1 and flags.tolist() == [0, 0, 0, 0]
    assert bool(core[LO:HI].any()) and not bool(core[LO:HI].all()) and int((labels[LO:HI] < 0).sum()) > 0


@pytest.mark.parametrize("limit", LIMITS)
def test_dbscan_clamps_ptr(dev, limit):
    from deepmetv2_amd import _native
    g, _perm = _grouped(_edges(CLAMP_SIZES, 0, thin=True), N, dev)
    runs = [_native._components(_t(p, dev), N, min_samples=3, count_self=True, lds_nodes=limit, **g)
            for p in (CLAMP_RAW, cr.ptr_of(CLAMP_SIZES))]
    assert _same(*runs) and runs[0][3].tolist() == [0, 0, 0, 0] and int(runs[0][2][1]) == 0


# ---- _condense --------------------------------------------------------------------------------------------------------------------
def _condense_inputs(dev, ptr):
    """beta, x on the lattice and the ranking of the events of `ptr` (a non-negative, non-decreasing one) as the operators
    form it; the ranking entries of the nodes no event owns are never read and hold -1."""
    from deepmetv2_amd import _native
    beta, x = cdr._lattice(np.random.default_rng(14), N, 3, 5)
    beta, x = _t(beta, dev), _t(x, dev)
    p = _t(ptr, dev)
    lo, hi = int(ptr[0]), int(ptr[-1])
    score = torch.where(beta > cdr.T_BETA, beta, float("-inf"))[lo:hi]
    order, _map = _native._topk(score, p - lo, p - lo, hi - lo)
    full = torch.full((N,), -1, dtype=torch.int64, device=dev)
    full[lo:hi] = order + lo
    return beta, x, full


@pytest.mark.parametrize("limit", LIMITS)
def test_condense(dev, limit):
    from deepmetv2_amd import _native
    beta, x, order = _condense_inputs(dev, PTR)
    kw = dict(t_beta=cdr.T_BETA, t_d=cdr.T_D, lds_nodes=limit)
    local, assoc, ncl, flags = _native._condense(beta, x, order, _t(PTR, dev), **kw)
    fill = torch.full((HEAD + TAIL,), -1, dtype=torch.int64)
    assert _eq(_unowned(local), fill) and _eq(_unowned(assoc), fill)
    s_local, s_assoc, s_ncl, s_flags = _native._condense(beta[LO:HI], x[LO:HI], order[LO:HI] - HEAD, _t(PTR - HEAD, dev), **kw)
    assert _eq(local[LO:HI], s_local) and _eq(assoc[LO:HI], _moved(s_assoc)) and _eq(ncl, s_ncl) and _eq(flags, s_flags)
    assert int(ncl[EMPTY]) == 0 and int(ncl.max()) > 1 and flags.tolist() == [0, 0]
    assert int((local[LO:HI] < 0).sum()) > 0                   # noise among the owned nodes too


@pytest.mark.parametrize("limit", LIMITS)
def test_condense_clamps_ptr(dev, limit):
    from deepmetv2_amd import _native
    clamped = cr.ptr_of(CLAMP_SIZES)
    beta, x, order = _condense_inputs(dev, clamped)
    runs = [_native._condense(beta, x, order, _t(p, dev), cdr.T_BETA, cdr.T_D, lds_nodes=limit) for p in (CLAMP_RAW, clamped)]
    assert _same(*runs) and runs[0][3].tolist() == [0, 0] and int(runs[0][2][1]) == 0

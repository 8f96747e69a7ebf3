"""Components and DBSCAN on the GPU: csrc/components.hip and deepmetv2_amd/components.py against scipy, sklearn and the
loop restatement of tests/components_reference.py.  Everything is an integer or a bool: equality, no tolerance.  The
cases and the conditions they meet are checked on the host in tests/test_components_host.py."""
import types

import numpy as np
import pytest
import torch

import components_reference as cr
import radius_periodic_reference as rp
from poisoned_alloc import run_both, to_bytes

pytestmark = pytest.mark.gpu

FORMS = ("padded", "counted", "list", "tensor")


@pytest.fixture(autouse=True)
def _drain():
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()
    yield
    dm.raise_deferred_errors()


@pytest.fixture(scope="module")
def ragged_labels():
    """scipy's canonical labels of the ragged batch, with and without the joining entry: computed once, never changed."""
    out = {}
    for g in (cr.ragged(), cr.ragged(cut_last=True)):
        out[g.name] = (g, cr.cc_scipy(g.N, g.tgt, g.src))
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _batch(dev, sizes):
    import deepmetv2_amd as dm
    sz = torch.tensor(sizes, dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sz.cumsum(0)])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sz).to(dev)
    dm.register_batch(batch, ptr.to(dev), len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    return batch


def _list_args(g, dev):
    rowptr, src, tgt, _perm = g.grouped()
    return dict(rowptr=_t(rowptr, dev), src=_t(src, dev), tgt=_t(tgt, dev))


def _form(g, form, dev, width=None):
    """The graph as one of the forms the operators take.  counted: the slots beyond a row's count hold an id outside the
    range -- they are never read; were they, the range flag would say so."""
    from deepmetv2_amd.graph import EdgeList, NeighborTable
    ptr = _t(cr.ptr_of(g.sizes), dev)
    width = int(g.counts().max()) if width is None else width
    if form == "padded":
        return NeighborTable(_t(g.table(width, np.random.default_rng(2)), dev), ptr, dense=False)
    if form == "counted":
        nbr = g.table(width)
        nbr[nbr < 0] = g.N + 5
        return NeighborTable(_t(nbr, dev), ptr, dense=False, cnt=_t(g.counts(), dev))
    if form == "list":
        a = _list_args(g, dev)
        return EdgeList(a["src"], a["tgt"], a["rowptr"], g.N)
    p = np.random.default_rng(4).permutation(len(g.tgt))
    return _t(g.edge_index[:, p], dev)


def _eq(got: torch.Tensor, want: np.ndarray) -> bool:
    w = torch.from_numpy(np.asarray(want))
    return got.dtype == w.dtype and torch.equal(got.cpu(), w)


# ---- connected components -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("list", "tensor"))
def test_ragged_batch_equals_scipy(dev, ragged_labels, form):
    import deepmetv2_amd as dm
    for g, want in ragged_labels.values():
        batch = _batch(dev, g.sizes)
        assert _eq(dm.connected_components(_form(g, form, dev), g.N, batch), want)
    # without a batch the whole input is one event: the same labels, every entry lies inside it
    g, want = ragged_labels["ragged"]
    assert _eq(dm.connected_components(_form(g, form, dev), g.N), want)


@pytest.mark.parametrize("limit", (0, 65, 64, 1))
def test_lds_and_workspace_forms_give_the_same_labels(dev, ragged_labels, limit):
    """limit 0 / 65: every event in LDS; 64: the 65- and the 300-node event through the workspace; 1: all but the
    one-node events."""
    from deepmetv2_amd import _native
    g, want = ragged_labels["ragged"]
    labels, core, ncl, flags = _native._components(_t(cr.ptr_of(g.sizes), dev), g.N, lds_nodes=limit, **_list_args(g, dev))
    assert _eq(labels, want) and core is None and ncl is None
    assert flags.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("limit", (0, 64))
def test_bit_reversed_path(dev, limit):
    from deepmetv2_amd import _native
    g = cr.bit_reversed_path()
    labels, _c, _n, flags = _native._components(_t(cr.ptr_of(g.sizes), dev), g.N, lds_nodes=limit, **_list_args(g, dev))
    assert _eq(labels, np.zeros(g.N, dtype=np.int64))
    assert flags.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("width", cr.TABLE_WIDTHS)
def test_every_graph_form_gives_the_same_labels(dev, width):
    import deepmetv2_amd as dm
    g = cr.width_graph(width)
    want = cr.cc_scipy(g.N, g.tgt, g.src)
    batch = _batch(dev, g.sizes)
    for form in FORMS:
        assert _eq(dm.connected_components(_form(g, form, dev, width), None, batch), want), form
    dm.raise_deferred_errors()          # no entry was out of range or across events: the counted form read no junk slot


def test_masks_equal_the_filtered_graph(dev):
    import deepmetv2_amd as dm
    g = cr.width_graph(16)
    edge_keep, node_keep = cr.masks(g)
    ptr = cr.ptr_of(g.sizes)
    batch = _batch(dev, g.sizes)
    keep = edge_keep & node_keep[g.tgt] & node_keep[g.src]
    want_both = cr.cc_scipy(g.N, g.tgt[keep], g.src[keep])
    want_both[~node_keep] = -1
    want_edge = cr.cc_scipy(g.N, g.tgt[edge_keep], g.src[edge_keep])
    assert np.array_equal(want_both, cr.cc_loops(g.N, g.tgt, g.src, ptr, edge_keep, node_keep)[0])
    assert not np.array_equal(want_edge, cr.cc_scipy(g.N, g.tgt, g.src))
    nm = _t(node_keep, dev)
    # the tensor: the mask in the caller's order, whatever order that is
    p = np.random.default_rng(4).permutation(len(g.tgt))
    ei = _t(g.edge_index[:, p], dev)
    assert _eq(dm.connected_components(ei, g.N, batch, edge_mask=_t(edge_keep[p], dev)), want_edge)
    assert _eq(dm.connected_components(ei, g.N, batch, edge_mask=_t(edge_keep[p], dev), node_mask=nm), want_both)
    # the list: grouped order
    _rowptr, _src, _tgt, perm = g.grouped()
    assert _eq(dm.connected_components(_form(g, "list", dev), None, batch, edge_mask=_t(edge_keep[perm], dev), node_mask=nm),
               want_both)
    # the tables: one value per slot; whatever an empty slot's value is, it is not read
    rows = g.rows()
    order = np.argsort(g.tgt, kind="stable")
    for form in ("padded", "counted"):
        table = _form(g, form, dev, 16)
        slots = table.nbr.cpu().numpy()
        filled = (slots >= 0) & (slots < g.N) if form == "padded" else np.arange(16)[None, :] < g.counts()[:, None]
        assert int(filled.sum()) == len(g.tgt) and sum(len(r) for r in rows) == len(g.tgt)
        for junk in (False, True):
            m = np.full((g.N, 16), junk, dtype=bool)
            m[filled] = edge_keep[order]            # row-major over the filled slots = the entries grouped by target
            assert _eq(dm.connected_components(table, None, batch, edge_mask=_t(m, dev), node_mask=nm), want_both), (form, junk)
    only_nodes = cr.cc_loops(g.N, g.tgt, g.src, ptr, None, node_keep)[0]
    assert _eq(dm.connected_components(_form(g, "padded", dev, 16), None, batch, node_mask=nm), only_nodes)


def test_entries_that_join_nothing_are_counted_and_reported(dev, ragged_labels):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    from deepmetv2_amd.graph import NeighborTable
    _g, want = ragged_labels["ragged"]
    for g, bad in cr.bad_entry_graphs():
        ptr = _t(cr.ptr_of(g.sizes), dev)
        for limit in (0, 64):
            labels, _c, _n, flags = _native._components(ptr, g.N, lds_nodes=limit, **_list_args(g, dev))
            assert _eq(labels, want) and flags.cpu().tolist() == bad + [0, 0], g.name
        assert _eq(dm.connected_components(_form(g, "list", dev), None, _batch(dev, g.sizes)), want)    # nothing raises here
        with pytest.raises(RuntimeError, match=r"connected_components: .*outside \[0, 496\)" if bad[0] else
                           "connected_components: .*two events"):
            dm.raise_deferred_errors()
    # a table: the spare column of a 17-wide table over the 16-wide graph holds the bad ids
    g = cr.width_graph(16)
    base = cr.cc_scipy(g.N, g.tgt, g.src)
    ptr = cr.ptr_of(g.sizes)
    nbr = g.table(17)
    nbr[ptr[3] + 2, 16], nbr[ptr[6] + 9, 16], nbr[ptr[5], 16] = g.N, -7, ptr[6] + 1
    labels, _c, _n, flags = _native._components(_t(ptr, dev), g.N, nbr=_t(nbr, dev))
    assert _eq(labels, base) and flags.cpu().tolist() == [2, 1, 0, 0]
    dm.dbscan_graph(NeighborTable(_t(nbr, dev), _t(ptr, dev), dense=False), 2)
    with pytest.raises(RuntimeError, match=r"dbscan_graph: .*outside \[0, 496\)"):
        dm.raise_deferred_errors()
    with pytest.raises(RuntimeError, match="dbscan_graph: .*two events"):         # each kind is a report of its own
        dm.raise_deferred_errors()


def test_empty_inputs(dev):
    import deepmetv2_amd as dm
    none = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    assert dm.connected_components(none, 5, _batch(dev, [3, 0, 2])).tolist() == [0, 1, 2, 3, 4]
    assert dm.connected_components(none, 0).numel() == 0
    assert dm.connected_components(none, 4).tolist() == [0, 1, 2, 3]
    labels, core = dm.dbscan_graph(none, 1, _batch(dev, [3, 0, 2]), count_self=True, return_core=True)
    assert labels.tolist() == [0, 1, 2, 3, 4] and core.tolist() == [True] * 5
    labels, core = dm.dbscan_graph(none, 2, _batch(dev, [3, 0, 2]), count_self=True, return_core=True)
    assert labels.tolist() == [-1] * 5 and core.tolist() == [False] * 5
    assert dm.largest_connected_components(none, 0).numel() == 0


# ---- largest components and pooling -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_components", (1, 2, 3))
def test_largest_components_equal_scipy(dev, ragged_labels, num_components):
    import deepmetv2_amd as dm
    for g, labels in ragged_labels.values():
        want = cr.largest_loops(labels, g.sizes, num_components)
        got = dm.largest_connected_components(_form(g, "tensor", dev), g.N, _batch(dev, g.sizes), num_components)
        assert _eq(got, want), g.name
    g, labels = ragged_labels["ragged_cut"]
    lo = int(cr.ptr_of(g.sizes)[4])
    if num_components == 1:             # the tie of the two 32-node paths goes to the one with the smaller root
        assert want[lo:lo + 32].all() and not want[lo + 32:lo + 64].any()


def test_pooling_takes_the_labels(dev, ragged_labels):
    import deepmetv2_amd as dm
    g, want = ragged_labels["ragged"]
    batch = _batch(dev, g.sizes)
    ei = _t(g.edge_index, dev)
    labels = dm.connected_components(ei, g.N, batch)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(g.N, 5, generator=gen).to(dev)
    data = types.SimpleNamespace(x=x, batch=batch, edge_index=ei, pos=torch.randn(g.N, 2, generator=gen).to(dev))
    ref = _t(want, dev)
    for pool in (dm.max_pool, dm.avg_pool):
        a, b = pool(labels, data), pool(ref, data)
        assert torch.equal(a.x, b.x) and torch.equal(a.batch, b.batch) and torch.equal(a.edge_index, b.edge_index)
        assert a.x.shape[0] == len(np.unique(want))
    node_map, _perm = dm.consecutive_cluster(labels)
    assert _eq(node_map, np.unique(want, return_inverse=True)[1].astype(np.int64))
    out, pooled = dm.max_pool_x(labels, x, batch)
    wmax = torch.full((len(np.unique(want)), 5), float("-inf")).scatter_reduce(
        0, torch.from_numpy(np.unique(want, return_inverse=True)[1]).view(-1, 1).expand(-1, 5), x.cpu(), "amax")
    assert torch.equal(out.cpu(), wmax)


# ---- DBSCAN over a graph ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sklearn_graph_labels():
    """{(with_self, min_samples): (labels over the batch, core)} from sklearn, event by event, numbered as the header says."""
    out = {}
    for with_self in (True, False):
        g = cr.dbscan_graph_case(with_self)
        for ms in cr.MIN_SAMPLES:
            labels, cores, before = [], [], 0
            for b in range(len(g.sizes)):
                lab, core = cr.dbscan_sklearn_event(g, b, ms, count_self=not with_self)
                labels.append(np.where(lab >= 0, lab + before, -1))
                cores.append(core)
                before += int(lab.max()) + 1 if len(lab) and lab.max() >= 0 else 0
            out[(with_self, ms)] = (np.concatenate(labels), np.concatenate(cores))
    return out


@pytest.mark.parametrize("with_self", (True, False))
@pytest.mark.parametrize("min_samples", cr.MIN_SAMPLES)
def test_dbscan_graph_equals_sklearn(dev, sklearn_graph_labels, min_samples, with_self):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    g = cr.dbscan_graph_case(with_self)
    want, want_core = sklearn_graph_labels[(with_self, min_samples)]
    batch = _batch(dev, g.sizes)
    for form in FORMS:
        labels, core = dm.dbscan_graph(_form(g, form, dev), min_samples, batch, count_self=not with_self, return_core=True)
        assert _eq(labels, want) and _eq(core, want_core), form
        assert _eq(dm.dbscan_graph(_form(g, form, dev), min_samples, batch, count_self=not with_self), want)
    # the workspace form: the same event-local numbers and counts
    ptr = _t(cr.ptr_of(g.sizes), dev)
    runs = [_native._components(ptr, g.N, min_samples=min_samples, count_self=not with_self, lds_nodes=limit,
                                **_list_args(g, dev)) for limit in (0, 12, 1)]
    for r in runs:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0])) and r[3].cpu().tolist() == [0, 0, 0, 0]
    loops = cr.dbscan_loops(g, min_samples, count_self=not with_self)
    assert runs[0][2].cpu().tolist() == loops[2] and np.array_equal(loops[0], want)
    dm.raise_deferred_errors()


# ---- DBSCAN over positions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.point_cases(), ids=lambda c: c.name)
def test_dbscan_equals_sklearn_on_float64(dev, case):
    import deepmetv2_amd as dm
    batch = _batch(dev, case.sizes)
    pos = torch.from_numpy(case.pos).float().to(dev)
    labels, core = dm.dbscan(pos, case.eps, case.min_samples, batch, max_num_neighbors=case.max_num_neighbors,
                             return_core=True)
    if case.overflows:
        with pytest.raises(RuntimeError, match="dbscan: .*max_num_neighbors=8"):
            dm.raise_deferred_errors()
        return
    dm.raise_deferred_errors()                          # rows of exactly max_num_neighbors hits are no error
    ptr, before = cr.ptr_of(case.sizes), 0
    for b in range(len(case.sizes)):
        want, want_core = case.sklearn_event(b)
        ours = labels[ptr[b]:ptr[b + 1]].cpu().numpy()
        assert ours.dtype == np.int64 and np.array_equal(np.where(ours >= 0, ours - before, -1), want), b
        assert np.array_equal(core[ptr[b]:ptr[b + 1]].cpu().numpy(), want_core), b
        before += int(want.max()) + 1 if len(want) and want.max() >= 0 else 0
    assert _eq(dm.dbscan(pos, case.eps, case.min_samples, batch, max_num_neighbors=case.max_num_neighbors), labels.cpu().numpy())


def test_dbscan_over_the_phi_seam(dev):
    import deepmetv2_amd as dm
    x, sizes, eps, min_samples, period = cr.periodic_case()
    hits = rp.radius_hits(x, cr.ptr_of(sizes), eps, period)
    assert max(len(h) for h in hits) <= 64
    g = cr.Graph("seam", sizes, np.concatenate([np.full(len(h), i) for i, h in enumerate(hits)]), np.concatenate(hits))
    want, want_core, _per = cr.dbscan_loops(g, min_samples, False)
    labels, core = dm.dbscan(_t(x, dev), eps, min_samples, _batch(dev, sizes), period=period, return_core=True)
    assert _eq(labels, want) and _eq(core, want_core)
    assert want.max() >= 1 and (want == -1).any()


# ---- whatever the buffers held, and no host read --------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((to_bytes(a) == to_bytes(b)).all())


@pytest.mark.parametrize("limit", (0, 12))
def test_same_outputs_whatever_the_buffers_held(dev, limit):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    g = cr.width_graph(16)
    ptr = _t(cr.ptr_of(g.sizes), dev)
    edge_keep, node_keep = cr.masks(g)
    _rowptr, _s, _tg, perm = g.grouped()
    counted = _form(g, "counted", dev, 16)
    d = cr.dbscan_graph_case(True)
    dptr = _t(cr.ptr_of(d.sizes), dev)
    dtab = _form(d, "padded", dev)
    calls = {
        "cc_list": lambda: _native._components(ptr, g.N, lds_nodes=limit, edge_mask=_t(edge_keep[perm], dev),
                                               node_mask=_t(node_keep, dev), **_list_args(g, dev)),
        "cc_counted": lambda: _native._components(ptr, g.N, lds_nodes=limit, nbr=counted.nbr, cnt=counted.cnt),
        "dbscan_list": lambda: _native._components(dptr, d.N, lds_nodes=limit, min_samples=5, **_list_args(d, dev)),
        "dbscan_padded": lambda: _native._components(dptr, d.N, lds_nodes=limit, min_samples=5, nbr=dtab.nbr),
    }
    if limit == 0:
        case = cr.point_cases()[0]
        pos = torch.from_numpy(case.pos).float().to(dev)
        batch = _batch(dev, case.sizes)
        calls["dbscan"] = lambda: dm.dbscan(pos, case.eps, case.min_samples, batch, return_core=True)
    for name, call in calls.items():
        clean = [t.cpu() for t in call() if t is not None]
        got = run_both(call)
        for pattern, tensors in got.items():
            assert len(tensors) == len(clean)
            for a, b in zip(clean, tensors):
                assert _same(a, b), (name, pattern)


def test_table_routes_make_no_host_read(dev):
    import deepmetv2_amd as dm
    g = cr.dbscan_graph_case(True)
    batch = _batch(dev, g.sizes)
    table = _form(g, "counted", dev)
    case = cr.point_cases()[0]
    pos = torch.from_numpy(case.pos).float().to(dev)
    pbatch = _batch(dev, case.sizes)

    def run():
        return (dm.connected_components(table, None, batch), dm.dbscan_graph(table, 5, batch, return_core=True),
                dm.dbscan(pos, case.eps, case.min_samples, pbatch, return_core=True))
    warm = run()                                        # library, pinned flags, workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = run()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(warm[0], again[0]) and torch.equal(warm[1][0], again[1][0]) and torch.equal(warm[2][0], again[2][0])

"""Components and DBSCAN without a GPU: the three statements of tests/components_reference.py against each other on every
case the GPU tests use, the conditions those cases are meant to meet, and the operators' argument checks (which run
before any device work: a CPU tensor gets as far as them)."""
import math

import numpy as np
import pytest
import torch

import components_reference as cr
import radius_periodic_reference as rp


# ---- the restatements agree ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", cr.cc_graphs(), ids=lambda g: g.name)
def test_loops_equal_scipy(g):
    labels, bad = cr.cc_loops(g.N, g.tgt, g.src, cr.ptr_of(g.sizes))
    assert bad == [0, 0]
    assert np.array_equal(labels, cr.cc_scipy(g.N, g.tgt, g.src))
    # grouping by target, and any other order of the entries, changes nothing
    _rowptr, src, tgt, _perm = g.grouped()
    assert np.array_equal(cr.cc_loops(g.N, tgt, src, cr.ptr_of(g.sizes))[0], labels)


def test_masked_loops_equal_scipy_on_the_filtered_graph():
    g = cr.ragged()
    edge_keep, node_keep = cr.masks(g)
    assert 0 < edge_keep.sum() < len(edge_keep) and 0 < node_keep.sum() < g.N
    got, _bad = cr.cc_loops(g.N, g.tgt, g.src, cr.ptr_of(g.sizes), edge_keep, node_keep)
    keep = edge_keep & node_keep[g.tgt] & node_keep[g.src]
    want = cr.cc_scipy(g.N, g.tgt[keep], g.src[keep])
    want[~node_keep] = -1
    assert np.array_equal(got, want)


@pytest.mark.parametrize("with_self", [True, False])
@pytest.mark.parametrize("min_samples", cr.MIN_SAMPLES)
def test_dbscan_rule_equals_sklearn(with_self, min_samples):
    g = cr.dbscan_graph_case(with_self)
    labels, core, per_event = cr.dbscan_loops(g, min_samples, count_self=not with_self)
    ptr = cr.ptr_of(g.sizes)
    before = 0
    for b in range(len(g.sizes)):
        want, want_core = cr.dbscan_sklearn_event(g, b, min_samples, count_self=not with_self)
        ours = labels[ptr[b]:ptr[b + 1]]
        assert np.array_equal(np.where(ours >= 0, ours - before, -1), want), b
        assert np.array_equal(core[ptr[b]:ptr[b + 1]], want_core), b
        assert per_event[b] == (want.max() + 1 if len(want) and want.max() >= 0 else 0)
        before += per_event[b]


def test_dbscan_rule_equals_sklearn_on_random_graphs():
    """The check the rule was adopted on, in small: random symmetric graphs, n in 1 .. 40, min_samples in 1 .. 6."""
    rng = np.random.default_rng(0)
    for _ in range(40):
        n = int(rng.integers(1, 41))
        a = np.triu(rng.random((n, n)) < rng.uniform(0.02, 0.3), 1)
        t, s = np.nonzero(a | a.T)
        g = cr.Graph("random", [n], t, s)
        ms = int(rng.integers(1, 7))
        labels, core, _per = cr.dbscan_loops(g, ms, count_self=True)
        want, want_core = cr.dbscan_sklearn_event(g, 0, ms, count_self=True)
        assert np.array_equal(labels, want) and np.array_equal(core, want_core)


# ---- the cases are what they are meant to be -------------------------------------------------------------------------------------
def test_the_ragged_batch_holds_its_conditions():
    g, cut = cr.ragged(), cr.ragged(cut_last=True)
    ptr = cr.ptr_of(g.sizes)
    assert g.sizes == [0, 1, 2, 63, 64, 65, 300, 1]
    ev = np.searchsorted(ptr, g.tgt, side="right") - 1
    assert np.array_equal(ev, np.searchsorted(ptr, g.src, side="right") - 1)          # every entry inside one event
    per_event = np.bincount(ev, minlength=len(g.sizes))
    assert per_event[2] == 0 and per_event[7] == 0 and g.sizes[2] > 0                  # events without an entry
    labels = cr.cc_scipy(g.N, g.tgt, g.src)
    touched = np.zeros(g.N, dtype=bool)
    touched[g.tgt] = touched[g.src] = True
    assert (~touched[ptr[5]:ptr[6]]).sum() >= 10                                       # isolated nodes beside a graph
    assert g.counts().max() == 300 and int(np.argmax(g.counts())) == ptr[6] + 7        # the hub's row
    assert (g.tgt == g.src).sum() >= 4                                                 # self entries
    pairs = list(zip(g.tgt.tolist(), g.src.tolist()))
    assert len(pairs) > len(set(pairs))                                                # duplicates
    assert any((s, t) not in set(pairs) for t, s in pairs if t != s)                   # one direction only
    # the last entry of the 64-node event joins its two halves, and is the last of its row and of the event when grouped
    last = int(np.flatnonzero(ev == 4)[-1])
    assert (g.tgt[last], g.src[last]) == (ptr[4] + 63, ptr[4] + 5) and g.tgt[ev == 4].max() == g.tgt[last]
    cut_labels = cr.cc_scipy(cut.N, cut.tgt, cut.src)
    a, b = cut_labels[ptr[4]:ptr[5]], labels[ptr[4]:ptr[5]]
    assert len(np.unique(a)) == 2 and len(np.unique(b)) == 1
    assert sorted(np.unique(a, return_counts=True)[1].tolist()) == [32, 32]            # a size tie for the largest component


def test_the_path_is_bit_reversed_and_one_component():
    g = cr.bit_reversed_path()
    assert g.N == 4096 and len(g.tgt) == 4095
    assert (cr.cc_scipy(g.N, g.tgt, g.src) == 0).all()
    assert np.median(np.abs(g.tgt - g.src)) > 1000          # neighbours on the path are far apart in id


@pytest.mark.parametrize("width", cr.TABLE_WIDTHS)
def test_width_graphs_fill_their_tables(width):
    g = cr.width_graph(width)
    counts = g.counts()
    assert counts.max() == width and counts.min() == 0
    ptr = cr.ptr_of(g.sizes)
    assert counts[ptr[7] - 1] == width                       # the last row of the 300-node event is full
    labels = cr.cc_scipy(g.N, g.tgt, g.src)
    assert len(np.unique(labels[ptr[6]:ptr[7]])) > 1        # still several components
    rng = np.random.default_rng(1)
    t = g.table(width, rng)
    assert sorted(t[t >= 0].tolist()) == sorted(g.src.tolist())


def test_bad_entry_graphs():
    for g, bad in cr.bad_entry_graphs():
        labels, got = cr.cc_loops(g.N, g.tgt, g.src, cr.ptr_of(g.sizes))
        assert got == bad
        base = cr.ragged()
        assert np.array_equal(labels, cr.cc_scipy(base.N, base.tgt, base.src))
        assert g.tgt.min() >= 0 and g.tgt.max() < g.N


def test_the_dbscan_graph_holds_its_conditions():
    for with_self in (True, False):
        g = cr.dbscan_graph_case(with_self)
        pairs = set(zip(g.tgt.tolist(), g.src.tolist()))
        assert len(pairs) == len(g.tgt) and all((s, t) in pairs for t, s in pairs)     # no duplicate, symmetric
        assert ((g.tgt == g.src).sum() == g.N) if with_self else not (g.tgt == g.src).any()
        labels, core, per_event = cr.dbscan_loops(g, 5, count_self=not with_self)
        rows = g.rows()
        # node 6: not core, core neighbours in two clusters, takes the one with the smaller root
        assert not core[6] and {int(labels[j]) for j in rows[6] if core[j]} == {0, 1} and labels[6] == 0
        ptr = cr.ptr_of(g.sizes)
        assert (labels[ptr[1]:ptr[2]] == -1).all() and per_event[1] == 0               # noise only
        assert per_event[2] == 1 and len(np.unique(labels[ptr[2]:ptr[3]])) == 1        # one cluster
        ev4 = labels[ptr[4]:ptr[5]]
        assert per_event[4] >= 2 and (ev4 == -1).any() and (~core[ptr[4]:ptr[5]] & (ev4 >= 0)).any()
        assert cr.dbscan_loops(g, 17, count_self=not with_self)[2][2] == 1


@pytest.mark.parametrize("case", cr.point_cases(), ids=lambda c: c.name)
def test_point_cases_sit_on_the_lattice(case):
    q = case.pos * 8
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < 2 ** 10       # exact in fp32, their squares and sums too
    eps2 = case.eps * case.eps
    assert abs(eps2 * 64 - (case.m + 0.5)) < 1e-9                            # no squared distance (k / 64) equals eps^2
    r32 = np.float32(case.eps)
    r2 = np.float32(r32 * r32)                                               # what the radius build compares against
    assert case.m / 64 < float(r2) < (case.m + 1) / 64
    ptr = cr.ptr_of(case.sizes)
    assert any(len(np.unique(case.pos[ptr[b]:ptr[b + 1]], axis=0)) < case.sizes[b] for b in range(len(case.sizes)))
    counts = case.neighbour_counts()
    assert case.min_samples <= case.max_num_neighbors
    if case.name == "exactly_full":
        assert counts.max() == case.max_num_neighbors and (counts == counts.max()).sum() == 8
    if case.overflows:
        assert counts.max() == case.max_num_neighbors + 1
    else:
        assert counts.max() <= case.max_num_neighbors
    if case.name in ("plane", "space"):                                      # clusters, border points and noise all occur
        labels = np.concatenate([case.sklearn_event(b)[0] for b in range(len(case.sizes))])
        core = np.concatenate([case.sklearn_event(b)[1] for b in range(len(case.sizes))])
        assert (labels == -1).any() and core.any() and (~core & (labels >= 0)).any()


def test_the_periodic_case_needs_the_seam():
    x, sizes, eps, min_samples, period = cr.periodic_case()
    ptr = cr.ptr_of(sizes)
    wrapped = rp.radius_hits(x, ptr, eps, period)
    plain = rp.radius_hits(x, ptr, eps, None)
    assert sum(len(h) for h in wrapped) > sum(len(h) for h in plain)
    assert np.abs(x[:, 1]).max() <= math.pi

    def run(hits):
        tgt = np.concatenate([np.full(len(h), i) for i, h in enumerate(hits)])
        return cr.dbscan_loops(cr.Graph("p", sizes, tgt, np.concatenate(hits)), min_samples, False)[0]
    assert not np.array_equal(run(wrapped), run(plain))


# ---- argument checks, before any device work -----------------------------------------------------------------------------------
def test_argument_checks_come_first():
    import deepmetv2_amd as dm
    ei = torch.tensor([[0, 1], [1, 2]])
    ok = torch.ones(2, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        dm.connected_components(torch.zeros(3, 2, dtype=torch.int64), 3)
    with pytest.raises(TypeError, match="int64"):
        dm.connected_components(ei.int(), 3)
    with pytest.raises(TypeError, match="NeighborTable"):
        dm.connected_components([[0, 1], [1, 2]], 3)
    with pytest.raises(TypeError, match="edge_mask must be a bool"):
        dm.connected_components(ei, 3, edge_mask=ok.float())
    with pytest.raises(ValueError, match=r"edge_mask must be \[2\]"):
        dm.connected_components(ei, 3, edge_mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(TypeError, match="node_mask must be a bool"):
        dm.connected_components(ei, 3, node_mask=torch.ones(3))
    with pytest.raises(ValueError, match="num_nodes"):
        dm.connected_components(ei, -1)
    with pytest.raises(TypeError, match="ptr"):
        dm.connected_components(ei, 3, ptr=torch.tensor([0, 3], dtype=torch.int32))
    for bad in (0, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="min_samples"):
            dm.dbscan_graph(ei, bad)
        with pytest.raises(ValueError, match="min_samples"):
            dm.dbscan(torch.zeros(4, 2), 0.5, bad)
    with pytest.raises(ValueError, match="max_num_neighbors >= 6"):
        dm.dbscan(torch.zeros(4, 2), 0.5, 6, max_num_neighbors=5)
    with pytest.raises(ValueError, match="max_num_neighbors"):
        dm.dbscan(torch.zeros(4, 2), 0.5, 1, max_num_neighbors=0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "0.5"):
        with pytest.raises(ValueError, match="eps"):
            dm.dbscan(torch.zeros(4, 2), bad)
    with pytest.raises(ValueError, match="pos"):
        dm.dbscan(torch.zeros(4), 0.5)
    for bad in (0, -1, 1.5, False):
        with pytest.raises(ValueError, match="num_components"):
            dm.largest_connected_components(ei, 3, num_components=bad)
    # a well-formed call gets past them and is stopped at the device
    with pytest.raises(RuntimeError, match="non-GPU"):
        dm.connected_components(ei, 3, edge_mask=ok)
    with pytest.raises(RuntimeError, match="non-GPU"):
        dm.dbscan_graph(ei, 2)


def test_names_are_public_and_add_no_autograd_function():
    import deepmetv2_amd as dm
    from deepmetv2_amd import components
    names = {"connected_components", "largest_connected_components", "dbscan_graph", "dbscan"}
    assert names <= set(dm.__all__) and all(n in dm.__doc__ for n in names)
    assert not any(isinstance(v, type) and issubclass(v, torch.autograd.Function) for v in vars(components).values())
    for n in names:
        assert "dmet.h" in dm.__dict__[n].__doc__ or "dbscan_graph" in dm.__dict__[n].__doc__ or "connected_components" in dm.__dict__[n].__doc__

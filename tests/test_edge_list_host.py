"""The edge list that a neighbour table hands to the operators (NeighborTable.edge_list), on the CPU stand-ins of
tests/fake_native.py.  A table built with `full_rows` (kNN with self loops, every event >= k nodes) is only EXPECTED to
have full rows: a non-finite query, or a node beyond the 1e10 squared-distance sentinel from the rest of its event, comes
out short.  The [2,E] view handed to the caller may carry -1 there (a deferred check reports it); the operators' edge list
must not: rowptr, src and tgt hold the valid entries only, as torch_cluster's result and oracle.ref_ops.knn_graph do."""
import torch

from fake_native import install


def _valid_entries(nbr):
    N, k = nbr.shape
    tgt = torch.arange(N, dtype=torch.int32).view(-1, 1).expand(N, k)
    keep = nbr >= 0
    return nbr[keep], tgt[keep]


def _check_edge_list(table, nbr):
    edges = table.edge_list()
    src, tgt = _valid_entries(nbr)
    assert int(edges.rowptr[-1]) == edges.src.numel() == edges.tgt.numel() == edges.num_edges == src.numel()
    assert edges.src.numel() == 0 or int(edges.src.min()) >= 0
    assert torch.equal(edges.src, src) and torch.equal(edges.tgt, tgt)
    deg = torch.bincount(tgt.long(), minlength=nbr.shape[0])
    assert torch.equal((edges.rowptr[1:] - edges.rowptr[:-1]).long(), deg)
    return edges


def test_full_rows_table_edge_list_drops_empty_slots(monkeypatch):
    install(monkeypatch)
    from deepmetv2_amd.graph import NeighborTable
    nbr = torch.tensor([[0, 1, 2],
                        [-1, -1, -1],       # empty row (a NaN query)
                        [2, -1, -1],        # only itself (a node beyond the sentinel distance)
                        [3, 0, 1],
                        [4, 3, -1],
                        [5, 4, 3]], dtype=torch.int32)
    ptr = torch.tensor([0, 3, 6])
    table = NeighborTable(nbr, ptr, dense=False, max_nodes=3, full_rows=True)
    edges = _check_edge_list(table, nbr)
    assert edges.num_edges == 12
    # the [2,E] view handed to the caller stays sized N k without a device read: the -1 slots are visible there
    ei = table.edge_index("source_to_target")
    assert ei.shape == (2, 18)
    assert torch.equal(ei[0], nbr.reshape(-1).long())
    assert torch.equal(ei[1], torch.arange(6).repeat_interleave(3))
    # ... and the operators' list did not change by asking for the view (nor the view by asking for the list first)
    assert table.edge_list() is edges and int(edges.rowptr[-1]) == 12


def test_full_rows_table_one_empty_row(monkeypatch):
    """The case of the issue: a 4 x 3 table with one empty row gives 9 edges, not 12."""
    install(monkeypatch)
    from deepmetv2_amd.graph import NeighborTable
    nbr = torch.tensor([[0, 1, 2], [1, 0, 2], [-1, -1, -1], [3, 2, 1]], dtype=torch.int32)
    table = NeighborTable(nbr, torch.tensor([0, 4]), dense=False, max_nodes=4, full_rows=True)
    assert table.edge_index().shape == (2, 12)       # view first: the list must not inherit its sizing
    edges = _check_edge_list(table, nbr)
    assert edges.num_edges == 9


def test_full_rows_table_without_short_rows(monkeypatch):
    install(monkeypatch)
    from deepmetv2_amd.graph import NeighborTable
    nbr = torch.tensor([[0, 1], [1, 0], [2, 3], [3, 2]], dtype=torch.int32)
    table = NeighborTable(nbr, torch.tensor([0, 2, 4]), dense=False, max_nodes=2, full_rows=True)
    edges = _check_edge_list(table, nbr)
    assert torch.equal(edges.rowptr, torch.arange(0, 10, 2, dtype=torch.int32))
    ei = table.edge_index()
    assert torch.equal(ei, torch.stack([edges.src.long(), edges.tgt.long()]))


def _short_row_coords():
    """three events of >= k = 4 nodes: a NaN query, an inf query, a node 2e5 away from the rest of its event"""
    g = torch.Generator().manual_seed(3)
    sizes = [9, 6, 5]
    x = torch.randn(sum(sizes), 3, generator=g)
    x[0, 1] = float("nan")
    x[10, 2] = float("inf")
    x[19, 0] += 2e5
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    return x, batch


def test_knn_table_short_rows_edge_list_matches_oracle(monkeypatch):
    install(monkeypatch)
    from deepmetv2_amd.cluster import knn_table
    from oracle import ref_ops
    x, batch = _short_row_coords()
    k = 4
    table = knn_table(x, k, batch)
    assert table.full_rows
    nbr = table.nbr
    assert bool((nbr[0] == -1).all()) and bool((nbr[10] == -1).all()) and nbr[19].tolist() == [19, -1, -1, -1]
    edges = _check_edge_list(table, nbr)
    ref = ref_ops.knn_graph(x, k, batch, loop=True)
    assert torch.equal(edges.src.long(), ref[0]) and torch.equal(edges.tgt.long(), ref[1])


def test_generic_edge_conv_on_short_rows_matches_oracle(monkeypatch):
    """An `nn` of no fused form over a full_rows table with short rows: the generic route (edge features, nn, segment
    reduction) on the stand-ins against the oracle's EdgeConv over the oracle's kNN graph; empty rows give 0, and the
    mean of a row that holds only its node divides by 1."""
    install(monkeypatch)
    import deepmetv2_amd as dm
    from oracle import ref_ops
    coords, batch = _short_row_coords()
    k = 4
    feats = torch.randn(coords.shape[0], 5, generator=torch.Generator().manual_seed(4))
    ref_ei = ref_ops.knn_graph(coords, k, batch, loop=True)
    for aggr in ("max", "add", "mean"):
        torch.manual_seed(1)
        nn = torch.nn.Sequential(torch.nn.Linear(10, 8), torch.nn.ReLU(), torch.nn.Linear(8, 6))
        conv = dm.EdgeConv(nn, aggr=aggr)
        nn.load_state_dict(conv.nn.state_dict())
        out = conv(feats, dm.knn_table(coords, k, batch))
        ref = ref_ops.edge_conv(feats, ref_ei, conv.nn, aggr)
        torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-6, msg=aggr)
        assert bool((out[0] == 0).all()) and bool((out[10] == 0).all()), aggr
        only_self = conv.nn(torch.cat([feats[19], torch.zeros(5)]).view(1, -1))[0]
        torch.testing.assert_close(out[19], only_self, rtol=1e-5, atol=1e-6, msg=aggr)

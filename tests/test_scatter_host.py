"""Index handling of the reduction layer without a GPU, on the CPU stand-ins of tests/fake_native.py: the checks of
batch vectors (graph.batch_info), of scatter indices (scatter_add / scatter_max) and of caller-supplied edge lists
(graph.edge_list_from_edge_index), and what a batch vector's call history may change.

A rejected input must never reach a kernel that reads through it.  The spy below lets only the entries that are safe
for any input run (batch_to_ptr writes ptr[0..B] whatever the vector holds; the reverse-index sort is safe for any key)
and fails the test if any other `_native` entry is called with a bad input on its way."""
import inspect

import pytest
import torch

import deepmetv2_amd as dm
import fake_native
from deepmetv2_amd import _native

SAFE_FOR_ANY_INPUT = {"batch_to_ptr", "reverse_index"}


@pytest.fixture(autouse=True)
def _fake(monkeypatch):
    fake_native.install(monkeypatch)
    # the global pools refuse CPU tensors up front; the stand-ins run on the CPU
    monkeypatch.setattr(_native, "_require_device", lambda *t: torch.device("cpu"))


@pytest.fixture
def spy(monkeypatch):
    """Records every public `_native` entry called; `spy.unsafe()` lists those outside SAFE_FOR_ANY_INPUT."""
    calls = []
    for name, fn in list(vars(_native).items()):
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ not in (_native.__name__,
                                                                                       fake_native.__name__):
            continue

        def wrapped(*a, _name=name, _fn=fn, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        monkeypatch.setattr(_native, name, wrapped)

    class Spy:
        def clear(self):
            calls.clear()

        def unsafe(self):
            return [c for c in calls if c not in SAFE_FOR_ANY_INPUT]

        def names(self):
            return list(calls)
    return Spy()


def _t(v, dtype=torch.int64):
    return torch.tensor(v, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------
# the stand-in of batch_to_ptr restates the kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,B", [([0, 0, 1, 3, 3], 4), ([0, 0, 1, 3, 3], 6), ([2, 2, 2], 3), ([0], 1)])
def test_batch_to_ptr_standin_matches_oracle_on_sorted_input(batch, B):
    from oracle import ref_ops
    b = _t(batch)
    assert torch.equal(fake_native.batch_to_ptr(b, B), ref_ops.batch_to_ptr(b, b.numel(), B))


@pytest.mark.parametrize("batch,B", [([-3, 0], 1), ([2, 0, 1, 0, 2], 3), ([5, -7, 9, 0], 2), ([-2, -1], 1),
                                     ([0, 0], 0), ([7, 7], 3)])
def test_batch_to_ptr_standin_writes_every_entry_and_nothing_else(batch, B):
    """The kernel's walk -1, batch..., B steps up past every b in [0, B]: all of ptr[0..B] is written, with positions
    in [0, N], for any vector (the stand-in asserts the first half itself)."""
    ptr = fake_native.batch_to_ptr(_t(batch), B)
    assert ptr.shape == (B + 1,)
    assert bool(((ptr >= 0) & (ptr <= len(batch))).all())


# ---------------------------------------------------------------------------------------------------------------
# B2: batch vectors are checked before any kernel reads through the ptr made of them
# ---------------------------------------------------------------------------------------------------------------
BAD_WITH_COUNT = [
    ([2, 0, 1, 0, 2], 3, "sorted"),         # unsorted, in range
    ([-3, 0], 1, r"\[0, 1\)"),              # negative first value
    ([0, 0, 1, 3, 3], 3, r"\[0, 3\)"),      # beyond the given count
    ([0, 1], 0, r"\[0, 0\)"),               # no event at all
]
BAD_INFERRED = [
    ([2, 0, 1, 0, 2], "sorted"),
    ([-3, 0], ">= 0"),
    ([-1, -1, 0], ">= 0"),
]


@pytest.mark.parametrize("batch,B,msg", BAD_WITH_COUNT)
def test_batch_info_rejects_bad_vector_with_count(spy, batch, B, msg):
    from deepmetv2_amd.graph import batch_info
    b = _t(batch)
    with pytest.raises(ValueError, match=msg):
        batch_info(b, b.numel(), b.device, B)
    assert spy.unsafe() == []
    # ... and the rejected count is not remembered: a later call without it sees the vector as it is
    if msg != "sorted" and batch[0] >= 0:
        assert batch_info(b, b.numel(), b.device).num_events == batch[-1] + 1


@pytest.mark.parametrize("batch,msg", BAD_INFERRED)
def test_batch_info_rejects_bad_vector_inferred(spy, batch, msg):
    from deepmetv2_amd.graph import batch_info
    b = _t(batch)
    with pytest.raises(ValueError, match=msg):
        batch_info(b, b.numel(), b.device)
    assert spy.names() == []        # refused on the first read, before the batch_to_ptr kernel


@pytest.mark.parametrize("batch,B,msg", BAD_WITH_COUNT)
def test_consumers_of_batch_info_reject_bad_vector(spy, batch, B, msg):
    b = _t(batch)
    N = b.numel()
    x = torch.randn(N, 11)
    w = torch.rand(N)
    calls = [lambda: dm.global_add_pool(x, b, size=B), lambda: dm.global_mean_pool(x, b, size=B),
             lambda: dm.global_max_pool(x, b, size=B), lambda: dm.met_reduce(w, x, b, num_events=B),
             lambda: dm.knn_table(x[:, :3].contiguous(), 1, b, num_events=B),
             lambda: dm.radius_table(x[:, :2].contiguous(), 0.5, b, num_events=B)]
    if B > 0:
        calls.append(lambda: dm.scatter.met_loss_from_weights(w, x, torch.randn(B, 11), b))
    for call in calls:
        spy.clear()
        with pytest.raises(ValueError, match=msg):
            call()
        assert spy.unsafe() == []


@pytest.mark.parametrize("batch,msg", BAD_INFERRED)
def test_consumers_of_batch_info_reject_bad_vector_inferred(spy, batch, msg):
    b = _t(batch)
    N = b.numel()
    x = torch.randn(N, 11)
    for call in (lambda: dm.global_add_pool(x, b), lambda: dm.global_max_pool(x, b),
                 lambda: dm.met_reduce(torch.rand(N), x, b), lambda: dm.knn_table(x[:, :3].contiguous(), 1, b)):
        spy.clear()
        with pytest.raises(ValueError, match=msg):
            call()
        assert spy.names() == []


def test_negative_sorted_index_never_reaches_a_kernel(spy):
    """Item 3 of the issue: a sorted batch such as [-3, 0] passed every host check, and the batch_to_ptr kernel wrote
    ptr[-2].  Now the inferred path refuses it before that kernel, and scatter_add (which groups an index it cannot
    use as a batch vector) raises IndexError before anything reads through it."""
    src = torch.tensor([1.0, 2.0])
    idx = _t([-3, 0])
    with pytest.raises(IndexError):
        dm.scatter_add(src, idx)
    assert spy.unsafe() == []
    spy.clear()
    with pytest.raises(IndexError):
        dm.scatter_add(src, idx, dim_size=4)
    assert spy.unsafe() == []


# ---------------------------------------------------------------------------------------------------------------
# B3: an unsorted in-range 1-D index takes the grouped path
# ---------------------------------------------------------------------------------------------------------------
def test_scatter_add_1d_unsorted_index():
    """Item 2 of the issue: torch_scatter gives [10, 4, 17]."""
    src = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0])
    idx = _t([2, 0, 1, 0, 2])
    assert dm.scatter_add(src, idx, dim_size=3).tolist() == [10.0, 4.0, 17.0]
    assert dm.scatter_add(src, idx.clone()).tolist() == [10.0, 4.0, 17.0]
    assert dm.scatter_add(src, idx.clone(), dim_size=5).tolist() == [10.0, 4.0, 17.0, 0.0, 0.0]


def test_scatter_add_1d_unsorted_backward():
    g = torch.Generator().manual_seed(2)
    src = torch.randint(-8, 9, (50,), generator=g).float().requires_grad_(True)
    idx = torch.randint(0, 7, (50,), generator=g)
    out = dm.scatter_add(src, idx, dim_size=9)
    ref = torch.zeros(9).index_add_(0, idx, src.detach())
    assert torch.equal(out.detach(), ref)
    coef = torch.randint(-8, 9, (9,), generator=g).float()
    (out * coef).sum().backward()
    assert torch.equal(src.grad, coef[idx])


# ---------------------------------------------------------------------------------------------------------------
# B5: scatter indices outside [0, dim_size) and per-column indices
# ---------------------------------------------------------------------------------------------------------------
OUT_OF_RANGE = [([0, 9, 1], 4), ([0, -5, 1], 4), ([0, 5, 1], 4), ([3, 7, 3], 4), ([0, 1], 0)]


@pytest.mark.parametrize("index,dim_size", OUT_OF_RANGE)
def test_scatter_2d_rejects_out_of_range_index(spy, index, dim_size):
    """Item 5 of the issue: with dim_size=4 the reverse-index sort keyed on the low 3 bits counted 9 in row 1 and -5
    in row 3 and dropped 5 and 7."""
    src = torch.randn(len(index), 3)
    idx = _t(index)
    for call in (lambda: dm.scatter_add(src, idx, dim=0, dim_size=dim_size),
                 lambda: dm.scatter_max(src, idx, dim=0, dim_size=dim_size),
                 lambda: dm.scatter_add(src, idx.view(-1, 1).expand(-1, 3), dim=0, dim_size=dim_size),
                 lambda: dm.scatter_add(src[:, 0].contiguous(), idx, dim_size=dim_size)):
        spy.clear()
        with pytest.raises(IndexError):
            call()
        assert spy.unsafe() == []


def test_scatter_negative_index_without_dim_size(spy):
    src = torch.randn(3, 2)
    for idx in (_t([0, -1, 2]), _t([-4, -2, -1])):
        for call in (lambda: dm.scatter_add(src, idx, dim=0), lambda: dm.scatter_max(src, idx, dim=0),
                     lambda: dm.scatter_add(src[:, 0].contiguous(), idx)):
            spy.clear()
            with pytest.raises(IndexError):
                call()
            assert spy.unsafe() == []


def test_scatter_2d_rejects_per_column_index(spy):
    """Item 4 of the issue: only column 0 of an [E,H] index was read."""
    s2 = torch.tensor([[1.0, 2.0], [4.0, 8.0]])
    i2 = _t([[0, 1], [1, 0]])
    for call in (lambda: dm.scatter_add(s2, i2, dim=0), lambda: dm.scatter_max(s2, i2, dim=0),
                 lambda: dm.scatter_add(s2, i2, dim=0, dim_size=2)):
        spy.clear()
        with pytest.raises(NotImplementedError):
            call()
        assert spy.unsafe() == []


def test_scatter_2d_index_shapes():
    g = torch.Generator().manual_seed(5)
    src = torch.randint(-8, 9, (40, 3), generator=g).float()
    idx = torch.randint(0, 6, (40,), generator=g)
    ref = torch.zeros(8, 3).index_add_(0, idx, src)
    for index in (idx, idx.view(-1, 1), idx.view(-1, 1).expand(-1, 3)):
        assert torch.equal(dm.scatter_add(src, index, dim=0, dim_size=8), ref)
    with pytest.raises(ValueError):
        dm.scatter_add(src, idx.view(-1, 1).expand(-1, 2), dim=0)
    with pytest.raises(ValueError):
        dm.scatter_max(src, idx[:-1], dim=0)
    with pytest.raises(TypeError):
        dm.scatter_max(src, idx.int(), dim=0)


# ---------------------------------------------------------------------------------------------------------------
# B6: caller-supplied edge lists
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ei", [[[0, 1, 5], [1, 2, 0]], [[0, 1, 2], [1, -1, 0]], [[0, 1, 2], [1, 2, 4]],
                                [[0, 2 ** 32 + 1, 2], [1, 2, 0]], [[0, 1, 2], [1, 2, -2 ** 32]]])
def test_edge_list_rejects_node_ids_out_of_range(spy, ei):
    """Item 5 of the issue, edge lists: ids >= N reached edge_features_kernel as gather addresses; ids that only alias a
    valid one after the int32 cast (2^32 + 1 -> 1) are caught as well."""
    from deepmetv2_amd.graph import edge_list_from_edge_index
    edge_index = _t(ei)
    for flow in ("source_to_target", "target_to_source"):
        spy.clear()
        with pytest.raises(ValueError, match=r"\[0, 4\)"):
            edge_list_from_edge_index(edge_index, 4, flow)
        assert spy.unsafe() == []
    for aggr in ("max", "add", "mean"):
        conv = dm.EdgeConv(torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ELU()), aggr=aggr)
        spy.clear()
        with pytest.raises(ValueError, match=r"\[0, 4\)"):
            conv(torch.randn(4, 3), edge_index)
        assert spy.unsafe() == []


def test_edge_list_in_range_unchanged():
    from deepmetv2_amd.graph import edge_list_from_edge_index
    ei = _t([[3, 0, 1, 2, 0], [0, 1, 0, 3, 3]])
    el = edge_list_from_edge_index(ei, 4, "source_to_target")
    assert el.tgt.tolist() == [0, 0, 1, 3, 3] and el.src.tolist() == [3, 1, 0, 2, 0]
    assert el.perm.tolist() == [0, 2, 1, 3, 4] and el.rowptr.tolist() == [0, 2, 3, 3, 5]
    with pytest.raises(ValueError):
        edge_list_from_edge_index(ei, 0, "source_to_target")


# ---------------------------------------------------------------------------------------------------------------
# B1: call history -- what one call passes never changes what another returns
# ---------------------------------------------------------------------------------------------------------------
def _fresh_sum(src, batch, **kw):
    return dm.scatter_add(src, batch.clone(), **kw)


def test_scatter_add_call_history():
    """Item 1 of the issue: after dim_size=6 the same tensor gave 6 entries without it, and after a call without
    dim_size, dim_size=3 gave 4 entries instead of failing."""
    src = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0])
    b = _t([0, 0, 1, 3, 3])
    assert dm.scatter_add(src, b, dim_size=6).tolist() == [3.0, 4.0, 0.0, 24.0, 0.0, 0.0]
    assert dm.scatter_add(src, b).tolist() == [3.0, 4.0, 0.0, 24.0]
    with pytest.raises(IndexError):
        dm.scatter_add(src, b, dim_size=3)
    assert torch.equal(dm.scatter_add(src, b, dim_size=6), _fresh_sum(src, b, dim_size=6))
    assert torch.equal(dm.scatter_add(src, b, dim_size=4), _fresh_sum(src, b))
    b2 = _t([0, 0, 1, 3, 3])          # the other order: without dim_size first
    assert dm.scatter_add(src, b2).shape == (4,)
    with pytest.raises(IndexError):
        dm.scatter_add(src, b2, dim_size=3)
    assert dm.scatter_add(src, b2, dim_size=6).tolist() == [3.0, 4.0, 0.0, 24.0, 0.0, 0.0]
    assert dm.scatter_add(src, b2).shape == (4,)


def test_global_pool_call_history():
    x = torch.randn(5, 3)
    b = _t([0, 0, 1, 3, 3])
    for pool in (dm.global_add_pool, dm.global_mean_pool, dm.global_max_pool):
        bb = b.clone()
        assert pool(x, bb, size=6).shape == (6, 3)
        assert torch.equal(pool(x, bb), pool(x, b.clone()))
        assert pool(x, bb).shape == (4, 3)
        with pytest.raises(ValueError):
            pool(x, bb, size=3)
        assert torch.equal(pool(x, bb, size=6), pool(x, b.clone(), size=6))


def test_met_reduce_and_knn_table_call_history():
    x = torch.randn(5, 11)
    w = torch.rand(5)
    b = _t([0, 0, 1, 3, 3])
    assert dm.met_reduce(w, x, b, num_events=6).shape == (6, 2)
    assert dm.met_reduce(w, x, b).shape == (4, 2)
    with pytest.raises(ValueError):
        dm.met_reduce(w, x, b, num_events=2)
    pos = x[:, :3].contiguous()
    b2 = b.clone()
    assert dm.knn_table(pos, 1, b2, num_events=7).ptr.shape == (8,)
    assert dm.knn_table(pos, 1, b2).ptr.shape == (5,)
    assert dm.knn_table(pos, 1, b2, num_events=6).ptr.tolist() == [0, 2, 3, 3, 5, 5, 5]


def test_registered_batch_keeps_its_count():
    """register_batch's count is the vector's own: it is not checked, and a caller's count does not replace it."""
    b = _t([0, 0, 1, 3, 3])
    dm.register_batch(b, _t([0, 2, 3, 3, 5, 5]), 5)
    src = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0])
    assert dm.scatter_add(src, b).tolist() == [3.0, 4.0, 0.0, 24.0, 0.0]
    assert dm.scatter_add(src, b, dim_size=7).tolist() == [3.0, 4.0, 0.0, 24.0, 0.0, 0.0, 0.0]
    assert dm.global_add_pool(torch.ones(5, 1), b).view(-1).tolist() == [2.0, 1.0, 0.0, 2.0, 0.0]

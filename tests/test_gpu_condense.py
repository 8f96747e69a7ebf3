"""Condensation clustering on the GPU: csrc/condense.hip and deepmetv2_amd/condense.py against the sequential statement of
tests/condense_reference.py.  Everything is an integer: equality, no tolerance.  The cases and the conditions they meet
are checked on the host in tests/test_condense_host.py."""
import numpy as np
import pytest
import torch

import condense_reference as cr
from poisoned_alloc import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _drain():
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()
    yield
    dm.raise_deferred_errors()


@pytest.fixture(scope="module")
def want():
    """name -> (case, the sequential statement's result): computed once per case, never changed."""
    memo = {}

    def get(case):
        if case.name not in memo:
            memo[case.name] = (case, cr.sequential(case))
        return memo[case.name]
    return get


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _batch(dev, sizes):
    import deepmetv2_amd as dm
    sz = torch.tensor(sizes, dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sz.cumsum(0)])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sz).to(dev)
    dm.register_batch(batch, ptr.to(dev), len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    return batch


def _eq(got: torch.Tensor, want_: np.ndarray) -> bool:
    w = torch.from_numpy(np.asarray(want_))
    return got.dtype == w.dtype and torch.equal(got.cpu(), w)


def _operands(case, dev):
    return _t(case.beta, dev), _t(case.x, dev), dict(t_beta=case.t_beta, t_d=case.t_d)


def _check_operators(case, ref, dev, **events):
    import deepmetv2_amd as dm
    beta, x, kw = _operands(case, dev)
    labels, assoc = dm.condensation_cluster(beta, x, return_assoc=True, **events, **kw)
    assert _eq(labels, ref.labels), case.name
    assert _eq(assoc, ref.assoc), case.name
    assert _eq(dm.condensation_cluster(beta, x, **events, **kw), ref.labels), case.name
    points, points_batch = dm.condensation_points(beta, x, **events, **kw)
    assert _eq(points, ref.points) and _eq(points_batch, ref.points_batch), case.name
    keep = labels >= 0
    assert torch.equal(points[labels[keep]], assoc[keep]), case.name
    return points_batch


def _native_run(case, dev, lds_nodes=0, order=None):
    """(local, assoc, ncl, flags, order) of the launch itself, over the ranking the operators form."""
    from deepmetv2_amd import _native
    beta, x, kw = _operands(case, dev)
    ptr = _t(cr.ptr_of(case.sizes), dev)
    if order is None:
        score = torch.where(beta > case.t_beta, beta, float("-inf"))
        order, _map = _native._topk(score, ptr, ptr, case.N)
    return (*_native._condense(beta, x, order, ptr, case.t_beta, case.t_d, lds_nodes=lds_nodes), order)


# ---- 1. the ragged batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 2, 3, 8))
def test_ragged_batch_equals_the_reference(dev, want, D):
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import batch_info
    case, ref = want(cr.ragged(D))
    batch = _batch(dev, case.sizes)
    points_batch = _check_operators(case, ref, dev, batch=batch)
    info = batch_info(points_batch, points_batch.numel(), dev)              # registered: no read
    assert _eq(info.ptr, cr.ptr_of(ref.counts)) and info.num_events == len(case.sizes)
    assert info.max_nodes == ref.counts.max() and info.min_nodes == ref.counts.min()
    _check_operators(case, ref, dev, ptr=_t(cr.ptr_of(case.sizes), dev))
    # an unregistered batch costs its read and gives the same
    plain = _t(np.repeat(np.arange(len(case.sizes)), case.sizes), dev)
    assert _eq(dm.condensation_cluster(_t(case.beta, dev), _t(case.x, dev), plain, t_beta=case.t_beta, t_d=case.t_d),
               ref.labels)
    if D == 1:                                                              # x as [N], beta as [N, 1]
        beta, x, kw = _operands(case, dev)
        assert _eq(dm.condensation_cluster(beta[:, None], x[:, 0], batch, **kw), ref.labels)


@pytest.mark.parametrize("D", (1, 3))
def test_a_single_event_needs_neither_batch_nor_ptr(dev, want, D):
    full = cr.ragged(D)
    lo, hi = cr.ptr_of(full.sizes)[-2:]
    case, ref = want(cr._case(f"ragged_d{D}_last", full.beta[lo:hi], full.x[lo:hi], [hi - lo]))
    assert case.N == 300
    _check_operators(case, ref, dev)


def test_the_random_batch_equals_the_reference(dev, want):
    case, ref = want(cr.random_batch())
    _check_operators(case, ref, dev, batch=_batch(dev, case.sizes))


def test_empty_inputs_and_an_unsorted_batch(dev):
    import deepmetv2_amd as dm
    none, nox = torch.zeros(0, device=dev), torch.zeros((0, 3), device=dev)
    labels, assoc = dm.condensation_cluster(none, nox, return_assoc=True)
    assert labels.dtype == torch.int64 and labels.numel() == 0 and assoc.numel() == 0
    points, points_batch = dm.condensation_points(none, nox, torch.zeros(0, dtype=torch.int64, device=dev))
    assert points.dtype == torch.int64 and points.numel() == 0 and points_batch.numel() == 0
    beta = torch.tensor([0.5, 0.75, 0.5], device=dev)
    x = torch.tensor([[0.0], [0.125], [4.0]], device=dev)
    batch = _batch(dev, [0, 2, 0, 1, 0])                                    # empty events in front, between and behind
    assert dm.condensation_cluster(beta, x, batch, t_d=0.3).tolist() == [0, 0, 1]
    points, points_batch = dm.condensation_points(beta, x, batch, t_d=0.3)
    assert points.tolist() == [1, 2] and points_batch.tolist() == [1, 3]
    with pytest.raises(ValueError, match="sorted"):
        dm.condensation_cluster(beta, x, torch.tensor([1, 0, 1], device=dev))


# ---- 2. the line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", (True, False))
def test_a_dead_entry_suppresses_nobody(dev, want, descending):
    case, ref = want(cr.line(descending))
    _check_operators(case, ref, dev)
    import deepmetv2_amd as dm
    beta, x, kw = _operands(case, dev)
    points, _pb = dm.condensation_points(beta, x, **kw)
    pos = np.arange(case.N)
    assert points.tolist() == (pos[::2] if descending else pos[::-1][::2]).tolist()


# ---- 3. window edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coincident", (False, True))
@pytest.mark.parametrize("count", cr.WINDOW_COUNTS)
def test_window_edges(dev, want, count, coincident):
    import deepmetv2_amd as dm
    case, ref = want(cr.window_edge(count, coincident))
    _check_operators(case, ref, dev, batch=_batch(dev, case.sizes))
    beta, x, kw = _operands(case, dev)
    got = dm.condensation_cluster(beta, x, _batch(dev, case.sizes), **kw).cpu().numpy()
    n = case.sizes[0]
    if coincident:
        assert np.all(got[:n] == 0)
    else:
        cand = np.flatnonzero(case.beta[:n] > np.float32(case.t_beta))
        rank = np.empty(count, dtype=np.int64)
        rank[np.argsort(-case.beta[cand], kind="stable")] = np.arange(count)
        assert np.array_equal(got[cand], rank)


# ---- 4. ties and specials -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cr.specials()))
def test_ties_and_specials(dev, want, name):
    import deepmetv2_amd as dm
    case, labels = cr.specials()[name]
    beta, x, kw = _operands(case, dev)
    assert dm.condensation_cluster(beta, x, **kw).tolist() == labels
    _check_operators(*want(case), dev)


# ---- 5. the radius edge -------------------------------------------------------------------------------------------------------
def test_the_radius_is_strict(dev, want):
    import deepmetv2_amd as dm
    case, ref = want(cr.radius_edge(1.0))
    _check_operators(case, ref, dev)
    beta, x, kw = _operands(case, dev)
    assert dm.condensation_cluster(beta, x, return_assoc=True, **kw)[1].tolist() == list(range(36))     # d2 == t_d2
    case, ref = want(cr.radius_edge(float(np.nextafter(np.float32(1), np.float32(2)))))
    _check_operators(case, ref, dev)
    assert ref.counts[0] < 36


# ---- 6. the state forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", (0, 64, 1))
def test_lds_and_workspace_forms_give_the_same_outputs(dev, want, limit):
    """limit 0: every event in LDS; 64: the 65-, 130- and 300-node events and the line through the workspace; 1: all but
    the one-node event."""
    for case in (cr.ragged(3), cr.ragged(8), cr.line(True), cr.line(False)):
        case, ref = want(case)
        local, assoc, ncl, flags, _order = _native_run(case, dev, lds_nodes=limit)
        assert _eq(local, ref.local) and _eq(assoc, ref.assoc) and _eq(ncl, ref.counts), (case.name, limit)
        assert flags.tolist() == [0, 0], (case.name, limit)


# ---- 7. an inconsistent ranking -----------------------------------------------------------------------------------------------
def test_a_ranking_entry_outside_its_event_is_skipped_and_counted(dev, want):
    """The kernel compares an entry against its event's range before it reads anything through it: ids of another event,
    below zero and beyond N are skipped alike, and flags[0] counts them."""
    case, ref = want(cr.inconsistent_ranking())
    ptr = cr.ptr_of(case.sizes)
    local, assoc, ncl, flags, order = _native_run(case, dev)
    assert _eq(local, ref.local) and flags.tolist() == [0, 0]
    lo, hi = int(ptr[1]), int(ptr[2])
    bad = order.clone()
    for slot, value in ((0, 3), (1, case.N + 7), (5, -1), (6, int(ptr[2]) + 1)):    # among the event's candidates
        bad[lo + slot] = value
    local2, assoc2, ncl2, flags2, _o = _native_run(case, dev, order=bad)
    assert flags2.tolist() == [4, 0]
    for a, b in ((local, local2), (assoc, assoc2)):
        assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[hi:], b[hi:])
    assert ncl2[0] == ncl[0] and ncl2[2] == ncl[2]
    # the middle event: every node still holds a number below the event's count or -1, and a point of the event or -1
    assert bool(((local2[lo:hi] >= -1) & (local2[lo:hi] < ncl2[1])).all())
    assert bool(((assoc2[lo:hi] == -1) | ((assoc2[lo:hi] >= lo) & (assoc2[lo:hi] < hi))).all())


# ---- 8. poisoned buffers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", (0, 64))
def test_same_outputs_whatever_the_buffers_held(dev, want, limit):
    import deepmetv2_amd as dm
    case, ref = want(cr.ragged(3))
    beta, x, kw = _operands(case, dev)
    batch = _batch(dev, case.sizes)
    calls = {"native": lambda: _native_run(case, dev, lds_nodes=limit)[:4]}
    if limit == 0:
        calls["operator"] = lambda: dm.condensation_cluster(beta, x, batch, return_assoc=True, **kw)
        calls["points"] = lambda: dm.condensation_points(beta, x, batch, **kw)
    for name, call in calls.items():
        clean = [t.cpu() for t in call()]
        for pattern, tensors in run_both(call).items():
            assert len(tensors) == len(clean)
            for a, b in zip(clean, tensors):
                assert a.dtype == b.dtype and torch.equal(a, b), (name, pattern)
    assert _eq(calls["native"]()[0], ref.local)


# ---- 9. no host read ----------------------------------------------------------------------------------------------------------
def test_a_registered_batch_makes_no_host_read(dev, want):
    import deepmetv2_amd as dm
    case, ref = want(cr.ragged(3))
    beta, x, kw = _operands(case, dev)
    batch = _batch(dev, case.sizes)
    ptr = _t(cr.ptr_of(case.sizes), dev)

    def run():
        return (dm.condensation_cluster(beta, x, batch, return_assoc=True, **kw), dm.condensation_cluster(beta, x, ptr=ptr, **kw))
    warm = run()                                        # library, pinned flags, workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = run()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(warm[0][0], again[0][0]) and torch.equal(warm[0][1], again[0][1]) and torch.equal(warm[1], again[1])
    assert _eq(again[0][0], ref.labels) and _eq(again[1], ref.labels)


# ---- 10. low-precision dtypes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16))
def test_low_precision_inputs_give_the_labels_of_their_upcasts(dev, want, dtype):
    """Lattice coordinates and beta in sixteenths are exact in both formats; values that are not are rounded by the caller's
    cast, and the operator sees the rounded ones either way."""
    import deepmetv2_amd as dm
    case, ref = want(cr.ragged(3))
    beta, x, kw = _operands(case, dev)
    lb, lx = beta.to(dtype), x.to(dtype)
    assert torch.equal(lb.float(), beta) and torch.equal(lx.float(), x)
    batch = _batch(dev, case.sizes)
    assert _eq(dm.condensation_cluster(lb, lx, batch, **kw), ref.labels)
    # values that do not fit: the labels of the upcast, not of the fp32 original
    g = torch.Generator(device="cpu").manual_seed(3)
    rb, rx = torch.rand(case.N, generator=g).to(dev), (torch.rand(case.N, 3, generator=g) * 2).to(dev)
    lb, lx = rb.to(dtype), rx.to(dtype)
    got = dm.condensation_cluster(lb, lx, batch, return_assoc=True, **kw)
    up = dm.condensation_cluster(lb.float(), lx.float(), batch, return_assoc=True, **kw)
    assert torch.equal(got[0], up[0]) and torch.equal(got[1], up[1])

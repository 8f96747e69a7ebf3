"""The fused add / sum / mean EdgeConv route for a single Linear message without a GPU: argument validation of the
include/dmet.h entries dmet_gather_sum_{table,csr,bwd}_f32 through ctypes, and the routing of CPU tensors on the
stand-ins of tests/fake_native.py (the generic route, as before)."""
import os
import shutil

import pytest
import torch

from fake_native import install

A = 16          # a non-NULL, 16-byte aligned stand-in address: every call below fails validation before any use of it


@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def _table(lib, P=A, Q=A, nbr=A, cnt=None, N=10, k=16, H=32, mean=0, out=A, deg=A):
    return lib.dmet_gather_sum_table_f32(P, Q, nbr, cnt, N, k, H, mean, out, deg, None)


def _csr(lib, P=A, Q=A, rowptr=A, src=A, N=10, H=32, mean=0, out=A, deg=A):
    return lib.dmet_gather_sum_csr_f32(P, Q, rowptr, src, N, H, mean, out, deg, None)


def _bwd(lib, g=A, deg=A, rev_ptr=A, rev_idx=A, tgt=None, N=10, k=16, H=32, mean=0, gP=A, gQ=A):
    return lib.dmet_gather_sum_bwd_f32(g, deg, rev_ptr, rev_idx, tgt, N, k, H, mean, gP, gQ, None)


def _rejects(lib, rc, entry, *words):
    assert rc == -22
    msg = lib.dmet_last_error().decode()
    assert entry in msg, msg
    for w in words:
        assert w in msg, msg


@pytest.mark.parametrize("fn,entry", [(_table, "dmet_gather_sum_table_f32"), (_csr, "dmet_gather_sum_csr_f32"),
                                      (_bwd, "dmet_gather_sum_bwd_f32")])
def test_rejects_bad_sizes(lib, fn, entry):
    _rejects(lib, fn(lib, N=-1), entry, "N=-1")
    for H in (0, 16, 48, 128):
        _rejects(lib, fn(lib, H=H), entry, f"H={H}")
    _rejects(lib, fn(lib, mean=2), entry, "mean=2")


def test_table_width_limits(lib):
    for k in (0, -3, 65):
        _rejects(lib, _table(lib, k=k), "dmet_gather_sum_table_f32", f"k={k}", "[1,64]")
    for k in (0, 1025):
        _rejects(lib, _table(lib, k=k, cnt=A), "dmet_gather_sum_table_f32", f"k={k}", "[1,1024]")
    for k in (-1, 1025):
        _rejects(lib, _bwd(lib, k=k), "dmet_gather_sum_bwd_f32", f"k={k}")


@pytest.mark.parametrize("arg", ["P", "Q", "nbr", "out", "deg"])
def test_table_rejects_null_pointers(lib, arg):
    _rejects(lib, _table(lib, **{arg: None}), "dmet_gather_sum_table_f32", "null pointer")


@pytest.mark.parametrize("arg", ["P", "Q", "rowptr", "out", "deg"])     # src may be NULL: E = 0
def test_csr_rejects_null_pointers(lib, arg):
    _rejects(lib, _csr(lib, **{arg: None}), "dmet_gather_sum_csr_f32", "null pointer")


@pytest.mark.parametrize("arg", ["g", "deg", "rev_ptr", "rev_idx", "gP", "gQ"])
def test_bwd_rejects_null_pointers(lib, arg):
    _rejects(lib, _bwd(lib, **{arg: None}), "dmet_gather_sum_bwd_f32", "null pointer")


def test_rejects_misaligned_rows(lib):
    _rejects(lib, _table(lib, P=A + 4), "dmet_gather_sum_table_f32", "aligned")
    _rejects(lib, _csr(lib, out=A + 8), "dmet_gather_sum_csr_f32", "aligned")
    _rejects(lib, _bwd(lib, gQ=A + 4), "dmet_gather_sum_bwd_f32", "aligned")


def test_empty_graph_is_a_no_op(lib):
    assert _table(lib, P=None, Q=None, nbr=None, out=None, deg=None, N=0) == 0
    assert _csr(lib, P=None, Q=None, rowptr=None, src=None, out=None, deg=None, N=0) == 0
    assert _bwd(lib, g=None, deg=None, rev_ptr=None, rev_idx=None, gP=None, gQ=None, N=0) == 0


# ---- routing on CPU tensors --------------------------------------------------------------------------------------------------
def _count_route(monkeypatch):
    from deepmetv2_amd import _native
    calls = []
    for name in ("gather_sum_table", "gather_sum_csr", "gather_sum_bwd"):
        monkeypatch.setattr(_native, name, lambda *a, _n=name, **k: calls.append(_n))
    return calls


@pytest.mark.parametrize("aggr", ["add", "sum", "mean"])
def test_cpu_tensors_keep_the_generic_route(monkeypatch, aggr):
    install(monkeypatch)
    calls = _count_route(monkeypatch)
    import deepmetv2_amd as dm
    from oracle import ref_ops
    g = torch.Generator().manual_seed(0)
    sizes = [40, 25]
    x = torch.randn(sum(sizes), 32, generator=g)
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes))
    torch.manual_seed(1)
    nn = torch.nn.Sequential(torch.nn.Linear(64, 32))
    for graph in ("knn_graph", "edge_index", "dynamic"):
        if graph == "dynamic":
            conv = dm.DynamicEdgeConv(nn, k=6, aggr=aggr)
            ei = ref_ops.knn_graph(x, 6, batch, loop=True)
            out = conv(x, batch)
        else:
            conv = dm.EdgeConv(nn, aggr=aggr)
            ei = dm.knn_graph(x, 6, batch, loop=True)
            out = conv(x, ei if graph == "knn_graph" else ei.clone())
        ref = ref_ops.edge_conv(x, ei, nn, aggr)
        torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    assert calls == []

"""The fp32 edge-MLP entries without a GPU: argument validation of include/dmet.h "fp32 edge MLP over any grouped edge
list" through ctypes, and the widths predicate."""
import os
import shutil

import pytest


@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def _fwd(lib, x=1, N=10, Hin=64, rowptr=1, src=1, tgt=1, E=20, W1=1, H1=96, W2=1, H2=64, aggr=1, bn=0, rm=None, rv=None,
         out=1, pq=1, agg=1, win=1, bnstat=1, ws=1, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dmet_edge_mlp_f32_workspace_bytes(max(N, 0), max(E, 0), Hin, H1, H2)
    return lib.dmet_edge_mlp_fwd_f32(x, N, Hin, rowptr, src, tgt, E, W1, None, H1, W2, None, H2, 1, aggr, bn, None, None,
                                     1e-5, 0.1, rm, rv, None, out, pq, agg, win, bnstat, ws, ws_bytes, None)


def _bwd(lib, x=1, N=10, Hin=64, E=20, srcptr=1, srcperm=1, H1=96, H2=64, aggr=1, bn=0, g_out=1, gpq=1, ws=1,
         ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dmet_edge_mlp_f32_workspace_bytes(max(N, 0), max(E, 0), Hin, H1, H2)
    return lib.dmet_edge_mlp_bwd_f32(x, N, Hin, 1, 1, 1, E, srcptr, srcperm, 1, H1, 1, None, H2, 1, aggr, bn, 1, 1, 1, 1,
                                     g_out, None, gpq, None, None, None, None, ws, ws_bytes, None)


@pytest.mark.parametrize("h", [16, 32, 64, 128])
def test_supported_drn_hidden(lib, h):
    from deepmetv2_amd import _native
    assert lib.dmet_edge_mlp_f32_supported(h, 3 * h // 2, h) == 1
    assert _native.edge_mlp_f32_supported(h, 3 * h // 2, h)
    assert lib.dmet_edge_mlp_f32_workspace_bytes(4500, 90000, h, 3 * h // 2, h) > 0


@pytest.mark.parametrize("widths", [(64, 96, 24), (64, 96, 48), (64, 96, 256), (129, 96, 64), (0, 96, 64), (64, 0, 64),
                                    (64, 193, 128), (16, 33, 16), (64, 96, 0)])
def test_supported_rejects(lib, widths):
    assert lib.dmet_edge_mlp_f32_supported(*widths) == 0
    assert lib.dmet_edge_mlp_f32_workspace_bytes(100, 100, *widths) == 0


def test_supported_edges_of_the_range(lib):
    assert lib.dmet_edge_mlp_f32_supported(1, 1, 16) == 1
    assert lib.dmet_edge_mlp_f32_supported(128, 192, 128) == 1
    assert lib.dmet_edge_mlp_f32_supported(128, 32, 16) == 1
    assert lib.dmet_edge_mlp_f32_supported(7, 128, 64) == 1


def test_workspace_grows_with_widths_not_with_edges(lib):
    a = lib.dmet_edge_mlp_f32_workspace_bytes(1000, 10_000, 64, 96, 64)
    b = lib.dmet_edge_mlp_f32_workspace_bytes(1000, 10_000_000, 64, 96, 64)
    assert a == b               # nothing per edge
    assert lib.dmet_edge_mlp_f32_workspace_bytes(1000, 10_000, 128, 192, 128) > a
    assert lib.dmet_edge_mlp_f32_workspace_bytes(-1, 10, 64, 96, 64) == 0


def test_fwd_argument_validation(lib):
    rc = _fwd(lib, H2=48)
    assert rc == -22 and b"unsupported widths" in lib.dmet_last_error() and b"H2=48" in lib.dmet_last_error()
    rc = _fwd(lib, N=-1)
    assert rc == -22 and b"N out of range" in lib.dmet_last_error()
    rc = _fwd(lib, E=-5)
    assert rc == -22 and b"E out of range" in lib.dmet_last_error()
    rc = _fwd(lib, aggr=3)
    assert rc == -22 and b"aggr" in lib.dmet_last_error()
    rc = _fwd(lib, bn=3)
    assert rc == -22 and b"bn must be" in lib.dmet_last_error()
    rc = _fwd(lib, bn=2)
    assert rc == -22 and b"running statistics" in lib.dmet_last_error()
    rc = _fwd(lib, bn=1, rm=1)
    assert rc == -22 and b"go together" in lib.dmet_last_error()
    rc = _fwd(lib, x=None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    rc = _fwd(lib, W2=None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    rc = _fwd(lib, src=None)
    assert rc == -22 and b"null edge array" in lib.dmet_last_error()
    rc = _fwd(lib, ws_bytes=16)
    assert rc == -22 and b"workspace too small" in lib.dmet_last_error()
    rc = _fwd(lib, ws=None)
    assert rc == -22 and b"workspace too small" in lib.dmet_last_error()
    rc = _fwd(lib, out=None)
    assert rc == -22 and b"null output" in lib.dmet_last_error()
    rc = _fwd(lib, aggr=0, win=None)
    assert rc == -22 and b"null output" in lib.dmet_last_error()
    rc = _fwd(lib, bn=1, E=0)
    assert rc == -22 and b"at least one edge" in lib.dmet_last_error()


def test_bwd_argument_validation(lib):
    rc = _bwd(lib, Hin=200)
    assert rc == -22 and b"unsupported widths" in lib.dmet_last_error()
    rc = _bwd(lib, N=-3)
    assert rc == -22 and b"N out of range" in lib.dmet_last_error()
    rc = _bwd(lib, g_out=None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    rc = _bwd(lib, gpq=None)
    assert rc == -22 and b"null pointer" in lib.dmet_last_error()
    rc = _bwd(lib, srcperm=None)
    assert rc == -22 and b"by-source" in lib.dmet_last_error()
    rc = _bwd(lib, ws_bytes=100)
    assert rc == -22 and b"workspace too small" in lib.dmet_last_error()
    rc = _bwd(lib, aggr=-1)
    assert rc == -22 and b"aggr" in lib.dmet_last_error()


def test_empty_input_reads_no_pointer(lib):
    # N = 0 needs no buffers: the forward writes nothing, the backward only the (here absent) weight gradients
    assert lib.dmet_edge_mlp_fwd_f32(None, 0, 64, None, None, None, 0, None, None, 96, None, None, 64, 1, 0, 0, None,
                                     None, 1e-5, 0.1, None, None, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.dmet_edge_mlp_bwd_f32(None, 0, 64, None, None, None, 0, None, None, None, 96, None, None, 64, 1, 0, 0,
                                     None, None, None, None, None, None, None, None, None, None, None, None, 0, None) == 0
    rc = _fwd(lib, N=0, E=3)
    assert rc == -22 and b"over no nodes" in lib.dmet_last_error()


def test_python_wrappers_refuse_host_tensors():
    import torch
    from deepmetv2_amd import _native
    x = torch.randn(4, 16)
    z = torch.zeros(5, dtype=torch.int32)
    e = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        _native.edge_mlp_fwd_f32(x, z, e, e, torch.randn(24, 32), None, torch.randn(16, 24), None, True, "add")

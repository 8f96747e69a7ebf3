"""The bf16 matrix-core edge-MLP entries without a GPU: the widths predicate and argument validation of include/dmet.h
"bf16 matrix-core edge MLP over any grouped edge list" through ctypes, the Python-side edge-array checks, and the
route selector's decisions (EdgeConv._forward_edge_mlp_bf16)."""
import os
import shutil
import types

import pytest
import torch


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
        ws_bytes = lib.dmet_edge_mlp_bf16_workspace_bytes(max(N, 0), max(E, 0), Hin, H1, H2)
    return lib.dmet_edge_mlp_fwd_bf16(x, N, Hin, rowptr, src, tgt, E, W1, None, H1, W2, None, H2, 1, aggr, bn, None, None,
                                      1e-5, 0.1, rm, rv, None, out, pq, agg, win, bnstat, ws, ws_bytes, None)


def _bwd(lib, x=1, N=10, Hin=64, E=20, srcptr=1, srcperm=1, H1=96, H2=64, aggr=1, bn=0, g_out=1, gpq=1, ws=1,
         ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dmet_edge_mlp_bf16_workspace_bytes(max(N, 0), max(E, 0), Hin, H1, H2)
    return lib.dmet_edge_mlp_bwd_bf16(x, N, Hin, 1, 1, 1, E, srcptr, srcperm, 1, H1, 1, None, H2, 1, aggr, bn, 1, 1, 1, 1,
                                      g_out, None, gpq, None, None, None, None, ws, ws_bytes, None)


# ---- widths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [32, 64, 128])
def test_supported_drn_hidden(lib, h):
    from deepmetv2_amd import _native
    assert lib.dmet_edge_mlp_bf16_supported(h, 3 * h // 2, h) == 1
    assert _native.edge_mlp_bf16_supported(h, 3 * h // 2, h)
    assert lib.dmet_edge_mlp_bf16_workspace_bytes(4500, 90000, h, 3 * h // 2, h) > 0


@pytest.mark.parametrize("widths", [(16, 24, 16), (64, 96, 24), (64, 96, 256), (129, 96, 64), (0, 96, 64), (64, 0, 64),
                                    (64, 40, 64), (64, 8, 32), (64, 80, 32), (128, 208, 128), (64, 96, 0)])
def test_supported_rejects(lib, widths):
    assert lib.dmet_edge_mlp_bf16_supported(*widths) == 0
    assert lib.dmet_edge_mlp_bf16_workspace_bytes(100, 100, *widths) == 0


def test_supported_edges_of_the_range(lib):
    assert lib.dmet_edge_mlp_bf16_supported(1, 16, 32) == 1
    assert lib.dmet_edge_mlp_bf16_supported(128, 64, 32) == 1
    assert lib.dmet_edge_mlp_bf16_supported(128, 192, 128) == 1
    assert lib.dmet_edge_mlp_bf16_supported(7, 112, 64) == 1
    assert lib.dmet_edge_mlp_bf16_supported(64, 128, 64) == 1
    assert lib.dmet_edge_mlp_bf16_supported(64, 144, 64) == 0      # H1 > 2 H2


def test_workspace_grows_with_widths_not_with_edges(lib):
    a = lib.dmet_edge_mlp_bf16_workspace_bytes(1000, 10_000, 64, 96, 64)
    b = lib.dmet_edge_mlp_bf16_workspace_bytes(1000, 10_000_000, 64, 96, 64)
    assert a == b > 0
    assert lib.dmet_edge_mlp_bf16_workspace_bytes(-1, 10, 64, 96, 64) == 0


# ---- C argument validation (no pointer is dereferenced: every call is refused before any launch) --------------------------
def test_forward_rejects_bad_arguments(lib):
    assert _fwd(lib, x=None) != 0
    assert _fwd(lib, rowptr=None) != 0
    assert _fwd(lib, W1=None) != 0
    assert _fwd(lib, W2=None) != 0
    assert _fwd(lib, src=None) != 0
    assert _fwd(lib, tgt=None) != 0
    assert _fwd(lib, out=None) != 0
    assert _fwd(lib, pq=None) != 0
    assert _fwd(lib, aggr=0, win=None) != 0
    assert _fwd(lib, ws=None) != 0
    assert _fwd(lib, ws_bytes=16) != 0
    assert _fwd(lib, H1=40, ws_bytes=1 << 20) != 0                 # unsupported widths
    assert _fwd(lib, H2=16, H1=16, ws_bytes=1 << 20) != 0
    assert _fwd(lib, aggr=3) != 0
    assert _fwd(lib, bn=3) != 0
    assert _fwd(lib, bn=2) != 0                                     # eval without running statistics
    assert _fwd(lib, rm=1) != 0                                     # running_mean without running_var
    assert _fwd(lib, bn=1, E=0) != 0                                # batch statistics over no edge
    assert _fwd(lib, N=-1) != 0
    assert _fwd(lib, N=0, E=5) != 0
    from deepmetv2_amd import _lib
    assert b"dmet_edge_mlp_fwd_bf16" in _lib.load().dmet_last_error()


def test_backward_rejects_bad_arguments(lib):
    assert _bwd(lib, x=None) != 0
    assert _bwd(lib, g_out=None) != 0
    assert _bwd(lib, gpq=None) != 0
    assert _bwd(lib, srcptr=None) != 0
    assert _bwd(lib, srcperm=None) != 0
    assert _bwd(lib, aggr=7) != 0
    assert _bwd(lib, H1=50, ws_bytes=1 << 20) != 0
    assert _bwd(lib, ws_bytes=8) != 0
    from deepmetv2_amd import _lib
    assert b"dmet_edge_mlp_bwd_bf16" in _lib.load().dmet_last_error()


def test_python_edge_arrays_are_checked():
    """the binding's checks before any device work: rowptr of N + 1 entries, src / tgt of one length, int32"""
    from deepmetv2_amd import _native
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    assert _native._edge_arrays(i32(11), i32(7), i32(7), 10) == 7
    with pytest.raises(ValueError, match="rowptr"):
        _native._edge_arrays(i32(10), i32(7), i32(7), 10)
    with pytest.raises(ValueError, match="differ in length"):
        _native._edge_arrays(i32(11), i32(7), i32(6), 10)
    with pytest.raises(TypeError):
        _native._edge_arrays(i32(11), torch.zeros(7, dtype=torch.int64), i32(7), 10)


# ---- the route selector --------------------------------------------------------------------------------------------------------
def _mlp(Hin, H1, H2, bn=None, act2=True):
    mods = [torch.nn.Linear(2 * Hin, H1), torch.nn.ELU(), torch.nn.Linear(H1, H2)] + ([torch.nn.ELU()] if act2 else [])
    if bn is not None:
        b = torch.nn.BatchNorm1d(H2)
        b.train(bn == "train")
        mods.append(b)
    return torch.nn.Sequential(*mods)


@pytest.fixture
def taken(monkeypatch, lib):
    """EdgeConv._forward_edge_mlp_bf16 on a stand-in device tensor: the list of calls that took the route"""
    from deepmetv2_amd import conv as conv_mod
    calls = []
    monkeypatch.setattr(conv_mod._EdgeMLP2Bf16Edges, "apply", staticmethod(lambda *a: calls.append(a) or "bf16 route"))

    def decide(nn, Hin=32, E=100, dtype=torch.float32, compute=torch.bfloat16, aggr="add"):
        import deepmetv2_amd as dm
        conv = dm.EdgeConv(nn, aggr=aggr)
        conv.compute_dtype = compute
        x = types.SimpleNamespace(is_cuda=True, dtype=dtype, shape=(50, Hin))
        edges = types.SimpleNamespace(num_edges=E)
        return conv._forward_edge_mlp_bf16(x, edges) == "bf16 route"
    return decide


def test_selector_takes_the_route(taken):
    for h in (32, 64, 128):
        assert taken(_mlp(h, 3 * h // 2, h), Hin=h)
        assert taken(_mlp(h, 3 * h // 2, h, bn="train"), Hin=h)
        assert taken(_mlp(h, 3 * h // 2, h, bn="eval", act2=False), Hin=h, aggr="max")
    assert taken(_mlp(32, 48, 32, bn="eval"), E=0)              # eval-mode BatchNorm over no edge: fine
    assert taken(_mlp(32, 48, 32), E=0, aggr="mean")


def test_selector_keeps_the_generic_route(taken, monkeypatch):
    assert not taken(_mlp(32, 48, 32), compute=torch.float32)    # fp32 compute
    assert not taken(_mlp(32, 48, 32), compute=None)             # neither bf16 nor autocast requested
    assert not taken(_mlp(32, 48, 16))                           # H2 = 16
    assert not taken(_mlp(32, 40, 32))                           # H1 not a multiple of 16
    assert not taken(_mlp(32, 48, 32), Hin=16)                   # in_features != 2 Hin
    assert not taken(_mlp(32, 48, 32), dtype=torch.float64)      # x not fp32
    assert not taken(torch.nn.Sequential(torch.nn.Linear(64, 32)))
    assert not taken(_mlp(32, 48, 32).double())                  # fp64 parameters
    assert not taken(_mlp(32, 48, 32, bn="train"), E=1)          # batch statistics over one edge: torch's error stays
    monkeypatch.setenv("DMET_EDGE_MLP_BF16", "0")
    assert not taken(_mlp(32, 48, 32))


def test_bf16_features_are_upcast_and_other_dtypes_raise():
    """EdgeConv / DynamicEdgeConv / knn_table: a bf16 x passes the dtype gate (upcast), fp16 still raises"""
    import deepmetv2_amd as dm
    conv = dm.EdgeConv(_mlp(4, 16, 32))
    ei = torch.zeros((2, 0), dtype=torch.int64)
    with pytest.raises(TypeError):
        conv(torch.zeros(3, 4, dtype=torch.float16), ei)
    with pytest.raises(TypeError):
        dm.knn_table(torch.zeros(3, 4, dtype=torch.float16), 2)
    with pytest.raises(TypeError):
        dm.DynamicEdgeConv(_mlp(4, 16, 32), k=2)(torch.zeros(3, 4, dtype=torch.float16))

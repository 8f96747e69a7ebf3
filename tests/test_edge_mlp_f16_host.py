"""The fp16 matrix-core edge-MLP entries without a GPU: the widths predicate and argument validation of include/dmet.h
"fp16 matrix-core edge MLP over any grouped edge list" through ctypes, the route selector's decisions
(EdgeConv._forward_edge_mlp_f16), and the dtype gates of the operators that take 16-bit inputs."""
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
        ws_bytes = lib.dmet_edge_mlp_f16_workspace_bytes(max(N, 0), max(E, 0), Hin, H1, H2)
    return lib.dmet_edge_mlp_fwd_f16(x, N, Hin, rowptr, src, tgt, E, W1, None, H1, W2, None, H2, 1, aggr, bn, None, None,
                                     1e-5, 0.1, rm, rv, None, out, pq, agg, win, bnstat, ws, ws_bytes, None)


def _bwd(lib, x=1, N=10, Hin=64, E=20, srcptr=1, srcperm=1, H1=96, H2=64, aggr=1, bn=0, g_out=1, gpq=1, ws=1,
         ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dmet_edge_mlp_f16_workspace_bytes(max(N, 0), max(E, 0), Hin, H1, H2)
    return lib.dmet_edge_mlp_bwd_f16(x, N, Hin, 1, 1, 1, E, srcptr, srcperm, 1, H1, 1, None, H2, 1, aggr, bn, 1, 1, 1, 1,
                                     g_out, None, gpq, None, None, None, None, ws, ws_bytes, None)


# ---- widths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [32, 64, 128])
def test_supported_drn_hidden(lib, h):
    from deepmetv2_amd import _native
    assert lib.dmet_edge_mlp_f16_supported(h, 3 * h // 2, h) == 1
    assert _native.edge_mlp_f16_supported(h, 3 * h // 2, h)
    assert lib.dmet_edge_mlp_f16_workspace_bytes(4500, 90000, h, 3 * h // 2, h) > 0


@pytest.mark.parametrize("widths", [(16, 24, 16), (64, 96, 24), (64, 96, 256), (129, 96, 64), (0, 96, 64), (64, 0, 64),
                                    (64, 40, 64), (64, 8, 32), (64, 80, 32), (128, 208, 128), (64, 96, 0)])
def test_supported_rejects(lib, widths):
    assert lib.dmet_edge_mlp_f16_supported(*widths) == 0
    assert lib.dmet_edge_mlp_f16_workspace_bytes(100, 100, *widths) == 0


def test_supported_edges_of_the_range(lib):
    assert lib.dmet_edge_mlp_f16_supported(1, 16, 32) == 1
    assert lib.dmet_edge_mlp_f16_supported(128, 64, 32) == 1
    assert lib.dmet_edge_mlp_f16_supported(128, 192, 128) == 1
    assert lib.dmet_edge_mlp_f16_supported(7, 112, 64) == 1
    assert lib.dmet_edge_mlp_f16_supported(64, 128, 64) == 1
    assert lib.dmet_edge_mlp_f16_supported(64, 144, 64) == 0       # H1 > 2 H2


def test_widths_and_workspace_equal_the_bf16_route(lib):
    for Hin in (1, 7, 32, 64, 128, 129):
        for H1 in (8, 16, 40, 48, 96, 144, 192, 208):
            for H2 in (16, 32, 64, 128, 256):
                assert lib.dmet_edge_mlp_f16_supported(Hin, H1, H2) == lib.dmet_edge_mlp_bf16_supported(Hin, H1, H2)
                assert (lib.dmet_edge_mlp_f16_workspace_bytes(1000, 20_000, Hin, H1, H2)
                        == lib.dmet_edge_mlp_bf16_workspace_bytes(1000, 20_000, Hin, H1, H2))


def test_workspace_grows_with_widths_not_with_edges(lib):
    a = lib.dmet_edge_mlp_f16_workspace_bytes(1000, 10_000, 64, 96, 64)
    b = lib.dmet_edge_mlp_f16_workspace_bytes(1000, 10_000_000, 64, 96, 64)
    assert a == b > 0
    assert lib.dmet_edge_mlp_f16_workspace_bytes(-1, 10, 64, 96, 64) == 0


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
    assert b"dmet_edge_mlp_fwd_f16" in _lib.load().dmet_last_error()


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
    assert b"dmet_edge_mlp_bwd_f16" in _lib.load().dmet_last_error()


def test_python_edge_arrays_are_checked():
    """the f16 bindings share the edge-array checks made before any device work: rowptr of N + 1 entries, src / tgt of
    one length, int32; the bindings refuse host tensors"""
    from deepmetv2_amd import _native
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    W1, W2 = torch.zeros(48, 64), torch.zeros(32, 48)
    with pytest.raises(RuntimeError, match="non-GPU"):
        _native.edge_mlp_fwd_f16(torch.zeros(10, 32), i32(11), i32(7), i32(7), W1, None, W2, None, True, "add")
    assert _native._edge_arrays(i32(11), i32(7), i32(7), 10) == 7
    with pytest.raises(TypeError):
        _native._edge_arrays(i32(11), torch.zeros(7, dtype=torch.int64), i32(7), 10)
    with pytest.raises(ValueError, match="rowptr"):
        _native._edge_arrays(i32(10), i32(7), i32(7), 10)
    with pytest.raises(ValueError, match="differ in length"):
        _native._edge_arrays(i32(11), i32(7), i32(6), 10)


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
    """EdgeConv._forward_edge_mlp_f16 / _bf16 on a stand-in device tensor: which route took the call (None: neither)"""
    from deepmetv2_amd import conv as conv_mod
    monkeypatch.setattr(conv_mod._EdgeMLP2F16Edges, "apply", staticmethod(lambda *a: "f16"))
    monkeypatch.setattr(conv_mod._EdgeMLP2Bf16Edges, "apply", staticmethod(lambda *a: "bf16"))

    def decide(nn, Hin=32, E=100, dtype=torch.float32, compute=torch.float16, aggr="add"):
        import deepmetv2_amd as dm
        conv = dm.EdgeConv(nn, aggr=aggr)
        conv.compute_dtype = compute
        x = types.SimpleNamespace(is_cuda=True, dtype=dtype, shape=(50, Hin))
        edges = types.SimpleNamespace(num_edges=E)
        a, b = conv._forward_edge_mlp_f16(x, edges), conv._forward_edge_mlp_bf16(x, edges)
        assert a is None or b is None
        return a or b
    return decide


def test_selector_takes_the_route(taken):
    for h in (32, 64, 128):
        assert taken(_mlp(h, 3 * h // 2, h), Hin=h) == "f16"
        assert taken(_mlp(h, 3 * h // 2, h, bn="train"), Hin=h) == "f16"
        assert taken(_mlp(h, 3 * h // 2, h, bn="eval", act2=False), Hin=h, aggr="max") == "f16"
    assert taken(_mlp(32, 48, 32, bn="eval"), E=0) == "f16"       # eval-mode BatchNorm over no edge: fine
    assert taken(_mlp(32, 48, 32), E=0, aggr="mean") == "f16"
    assert taken(_mlp(32, 48, 32), compute=torch.bfloat16) == "bf16"


def test_selector_keeps_the_generic_route(taken, monkeypatch):
    assert taken(_mlp(32, 48, 32), compute=torch.float32) is None     # fp32 compute
    assert taken(_mlp(32, 48, 32), compute=None) is None              # no 16-bit dtype, no autocast
    assert taken(_mlp(32, 48, 16)) is None                            # H2 = 16
    assert taken(_mlp(32, 40, 32)) is None                            # H1 not a multiple of 16
    assert taken(_mlp(32, 48, 32), Hin=16) is None                    # in_features != 2 Hin
    assert taken(_mlp(32, 48, 32), dtype=torch.float64) is None       # x not fp32
    assert taken(torch.nn.Sequential(torch.nn.Linear(64, 32))) is None
    assert taken(_mlp(32, 48, 32).double()) is None                   # fp64 parameters
    assert taken(_mlp(32, 48, 32, bn="train"), E=1) is None           # batch statistics over one edge: torch's error
    monkeypatch.setenv("DMET_EDGE_MLP_F16", "0")
    assert taken(_mlp(32, 48, 32)) is None
    assert taken(_mlp(32, 48, 32), compute=torch.bfloat16) == "bf16"  # the bf16 switch is its own


def test_requested_dtype_follows_compute_dtype_then_autocast():
    import deepmetv2_amd as dm
    conv = dm.EdgeConv(_mlp(4, 16, 32))
    assert conv._wants_16bit() is None and not conv._wants_bf16()
    for dt in (torch.float16, torch.bfloat16):
        conv.compute_dtype = dt
        assert conv._wants_16bit() == dt and conv._wants_bf16() == (dt == torch.bfloat16)
    conv.compute_dtype = torch.float32
    assert conv._wants_16bit() is None


def test_16bit_features_pass_the_dtype_gate_and_others_raise(monkeypatch):
    """The graph builders upcast a bf16 x always and an fp16 x while fp16 autocast is on; EdgeConv takes an fp16 x when
    fp16 is requested (autocast or compute_dtype).  Without such a request fp16 still raises, and fp64 always does."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import cluster
    conv = dm.EdgeConv(_mlp(4, 16, 32))
    ei = torch.zeros((2, 0), dtype=torch.int64)
    y = cluster._check_x(torch.ones(3, 4, dtype=torch.bfloat16))
    assert y.dtype == torch.float32 and torch.equal(y, torch.ones(3, 4))
    with pytest.raises(TypeError):
        cluster._check_x(torch.ones(3, 4, dtype=torch.float16))
    assert not conv._takes_fp16()
    conv.compute_dtype = torch.float16
    assert conv._takes_fp16()
    conv.compute_dtype = None
    monkeypatch.setattr(cluster, "fp16_autocast", lambda: True)     # as under torch.autocast("cuda")
    y = cluster._check_x(torch.ones(3, 4, dtype=torch.float16))
    assert y.dtype == torch.float32 and torch.equal(y, torch.ones(3, 4))
    from deepmetv2_amd import conv as conv_mod
    monkeypatch.setattr(conv_mod, "fp16_autocast", lambda: True)
    assert conv._takes_fp16()
    with pytest.raises(TypeError):
        conv(torch.zeros(3, 4, dtype=torch.float64), ei)
    with pytest.raises(TypeError):
        dm.knn_table(torch.zeros(3, 4, dtype=torch.float64), 2)
    with pytest.raises(TypeError):
        dm.radius_table(torch.zeros(3, 2, dtype=torch.float64), 0.4)
    with pytest.raises(TypeError):
        dm.DynamicEdgeConv(_mlp(4, 16, 32), k=2)(torch.zeros(3, 4, dtype=torch.float64))

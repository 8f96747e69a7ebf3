"""The three fused edge-MLP routes (f32, bf16, f16) behind one host path, without a GPU: every rejection names the entry
that was called, the workspace sizes are the ones of the layout before it had one owner, and the Python names that tests
and tools patch are route-bound functions and classes of their own."""
import os
import shutil
import types

import pytest
import torch

ROUTES = ("f32", "bf16", "f16")


@pytest.fixture(scope="module")
def lib():
    from deepmetv2_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libdmet_hip.so not built and no hipcc here")
        build.build_hip()
    return _lib.load()


def _call(lib, route, which, N=10, Hin=64, E=20, H1=96, H2=64, aggr=1, bn=0, src=1, short=0):
    """dmet_edge_mlp_{fwd,bwd}_{route} over stand-in pointers (every call here is rejected before any is read)"""
    ws_bytes = getattr(lib, f"dmet_edge_mlp_{route}_workspace_bytes")(max(N, 0), max(E, 0), Hin, H1, H2) - short
    fn = getattr(lib, f"dmet_edge_mlp_{which}_{route}")
    if which == "fwd":
        return fn(1, N, Hin, 1, src, 1, E, 1, None, H1, 1, None, H2, 1, aggr, bn, None, None, 1e-5, 0.1, None, None, None,
                  1, 1, 1, 1, 1, 1, ws_bytes, None)
    return fn(1, N, Hin, 1, src, 1, E, 1, 1, 1, H1, 1, None, H2, 1, aggr, bn, 1, 1, 1, 1, 1, None, 1, None, None, None, None,
              1, ws_bytes, None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("route", ROUTES)
def test_every_rejection_names_the_entry_called(lib, route, which):
    entry = f"dmet_edge_mlp_{which}_{route}".encode()
    cases = [(dict(N=-1), b"N out of range"), (dict(N=2147483647 // 384), b"N out of range"),
             (dict(H2=48), b"unsupported widths"), (dict(Hin=129), b"unsupported widths"),
             (dict(aggr=3), b"aggr must be"), (dict(aggr=-1), b"aggr must be"), (dict(bn=3), b"bn must be"),
             (dict(short=1), b"workspace too small"), (dict(src=None), b"null edge array")]
    if which == "fwd":
        cases.append((dict(bn=2), b"eval mode needs running statistics"))
    if route != "f32":
        cases.append((dict(H1=40, H2=32, Hin=32), b"unsupported widths"))      # H1 not a multiple of 16: fp32 only
    for kw, what in cases:
        assert _call(lib, route, which, **kw) == -22, kw
        msg = lib.dmet_last_error()
        assert msg.startswith(entry + b":") and what in msg, (kw, msg)


@pytest.mark.parametrize("route", ROUTES)
def test_empty_input_reads_no_pointer(lib, route):
    fwd, bwd = getattr(lib, f"dmet_edge_mlp_fwd_{route}"), getattr(lib, f"dmet_edge_mlp_bwd_{route}")
    assert fwd(None, 0, 64, None, None, None, 0, None, None, 96, None, None, 64, 1, 0, 0, None, None, 1e-5, 0.1, None, None,
               None, None, None, None, None, None, None, 0, None) == 0
    assert bwd(None, 0, 64, None, None, None, 0, None, None, None, 96, None, None, 64, 1, 0, 0, None, None, None, None, None,
               None, None, None, None, None, None, None, 0, None) == 0


# dmet_edge_mlp_*_workspace_bytes as the build before this layout had one owner returned them: by (Hin, H1, H2), for every
# (N, E) -- nothing in the workspace is per node or per edge
WORKSPACE_BYTES = {(16, 24, 16): 855808, (32, 48, 32): 3290368, (64, 96, 64): 12896000, (128, 192, 128): 51055872,
                   (7, 112, 64): 14950400}


@pytest.mark.parametrize("route", ROUTES)
def test_workspace_bytes_are_the_recorded_ones(lib, route):
    fn = getattr(lib, f"dmet_edge_mlp_{route}_workspace_bytes")
    for widths, nbytes in WORKSPACE_BYTES.items():
        if widths[2] == 16 and route != "f32":
            nbytes = 0                                  # H2 = 16 is an fp32 width only
        for N, E in ((1, 0), (1000, 10_000), (4500, 10_000_000)):
            assert fn(N, E, *widths) == nbytes, (widths, N, E)
    assert fn(-1, 10, 64, 96, 64) == 0 and fn(10, -1, 64, 96, 64) == 0
    assert fn(100, 100, 64, 96, 48) == 0 and fn(100, 100, 129, 96, 64) == 0 and fn(100, 100, 64, 193, 128) == 0
    assert fn(100, 100, 64, 100, 64) == (13422592 if route == "f32" else 0)     # H1 = 100: no multiple of 16
    assert fn(100, 100, 64, 8, 64) == (1316096 if route == "f32" else 0)        # H1 = 8: below one MFMA block


def test_python_names_carry_their_route():
    from deepmetv2_amd import _native, conv
    for route in ROUTES:
        for stem in ("edge_mlp_fwd_{}", "edge_mlp_bwd_{}", "edge_mlp_{}_supported"):
            fn = getattr(_native, stem.format(route))
            assert fn.__name__ == stem.format(route) and f"_{route}" in fn.__doc__
    for name, route in (("_EdgeMLP2F32", "F32"), ("_EdgeMLP2Bf16Edges", "Bf16"), ("_EdgeMLP2F16Edges", "F16")):
        cls = getattr(conv, name)
        assert issubclass(cls, torch.autograd.Function) and cls.__name__ == cls.__qualname__ == name and route in name
        assert cls.__doc__ and f"DMET_EDGE_MLP_{route.upper()}=0" in cls.__doc__
    assert len({conv._EdgeMLP2F32, conv._EdgeMLP2Bf16Edges, conv._EdgeMLP2F16Edges}) == 3
    with pytest.raises(TypeError, match="edge_mlp_f16: src"):
        z = torch.zeros(5, dtype=torch.int32)
        _native._edge_arrays(z, torch.zeros(3, dtype=torch.int64), z, 4, "f16")


def _mlp(Hin=32, H1=48, H2=32):
    return torch.nn.Sequential(torch.nn.Linear(2 * Hin, H1), torch.nn.ELU(), torch.nn.Linear(H1, H2))


class _OnGpu(torch.Tensor):
    """a host tensor that passes the selector's device gate; the native entry it would reach is patched"""
    is_cuda = True


def test_a_patched_native_entry_is_the_one_edgeconv_calls(lib, monkeypatch):
    """EdgeConv -> selector -> autograd class -> _native.edge_mlp_fwd_bf16 looked up at call time, as the GPU tests' _count
    helpers rely on"""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    seen = []

    def fake(x, *a, **k):
        seen.append(1)
        return torch.zeros((x.shape[0], 32)), (torch.zeros(1), torch.zeros(1), None, torch.zeros(1))
    monkeypatch.setattr(_native, "edge_mlp_fwd_bf16", fake)
    monkeypatch.setattr(_native, "edge_mlp_fwd_f16", lambda *a, **k: pytest.fail("the f16 entry was called"))
    monkeypatch.setattr(_native, "edge_mlp_fwd_f32", lambda *a, **k: pytest.fail("the f32 entry was called"))
    layer = dm.EdgeConv(_mlp(), aggr="add")
    layer.compute_dtype = torch.bfloat16
    edges = types.SimpleNamespace(rowptr=None, src=None, tgt=None, num_edges=5)
    out = layer._forward_edge_list(torch.zeros(4, 32).as_subclass(_OnGpu), edges)
    assert len(seen) == 1 and tuple(out.shape) == (4, 32)


@pytest.mark.parametrize("route", ROUTES)
def test_each_selector_refuses_the_other_two_dtypes(lib, monkeypatch, route):
    import deepmetv2_amd as dm
    from deepmetv2_amd import conv
    for cls in (conv._EdgeMLP2F32, conv._EdgeMLP2Bf16Edges, conv._EdgeMLP2F16Edges):
        monkeypatch.setattr(cls, "apply", staticmethod(lambda *a, _n=cls.__name__: _n))
    layer = dm.EdgeConv(_mlp(), aggr="add")
    x = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=(50, 32))
    edges = types.SimpleNamespace(num_edges=100)
    taken = {"f32": "_EdgeMLP2F32", "bf16": "_EdgeMLP2Bf16Edges", "f16": "_EdgeMLP2F16Edges"}
    request = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    select = getattr(layer, f"_forward_edge_mlp_{route}")
    for asked, dtype in request.items():
        layer.compute_dtype = dtype
        assert select(x, edges) == (taken[route] if asked == route else None), (route, asked)
    layer.compute_dtype = request[route]
    monkeypatch.setenv(f"DMET_EDGE_MLP_{route.upper()}", "0")
    assert select(x, edges) is None

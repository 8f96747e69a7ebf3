"""The per-node chain (encoder, BatchNorm, head and the fused hand-overs between them) on every route its dispatch can
take, each held to the float64 references of tests/per_node_reference.py at the bars of tests/test_gpu_parity.py.

The C entries choose their kernel per call from where the operands sit in memory: the matrix-core kernels need the
embedding tables (encoder) or W1, b1, W2 (head) on 16-byte boundaries and the scalar-weight ("valu") kernels take over
otherwise; dmet_bn_head_fwd_f32 and dmet_encode_bn_bwd_f32 launch nothing when one of their pointers is unaligned and
Python runs the two separate steps.  Freshly allocated tensors are always aligned; parameters that are views into a flat
buffer without padding are not.  `misaligned` builds such views.

Which route ran ("returns a result", "returns None", "the bits of the valu switch") is a property of the default
dispatch: tests asserting it skip, with the reason, when tools/toggle_sweep.sh has forced one of the switches for the
whole run.  The comparisons with the references run under every switch.
"""
import functools
import os

import pytest
import torch

import per_node_reference as pn
from per_node_reference import close, misaligned

pytestmark = pytest.mark.gpu


def _default_route_only(*switches):
    for name in switches:
        if os.environ.get(name) == "valu":
            pytest.skip(f"{name}=valu: the scalar-weight kernels are forced for the whole run; which route the default "
                        "dispatch takes is not in question")


def _equal(a, b, what):
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ in their bits"


def _spy(monkeypatch, module, name):
    """Record what module.name returns (the dense layer looks the function up on the module at call time)."""
    real, seen = getattr(module, name), []

    def wrapper(*args, **kwargs):
        seen.append(real(*args, **kwargs))
        return seen[-1]
    monkeypatch.setattr(module, name, wrapper)
    return seen


def _placed(cpu_tensors, dev, where):
    """Device leaves of `cpu_tensors`; where = {index: byte offset} puts those at that offset from a 16-byte boundary."""
    out = []
    for i, t in enumerate(cpu_tensors):
        t = t.to(dev)
        assert t.data_ptr() % 16 == 0
        if i in where:
            t = misaligned(t, where[i])
        out.append(t.detach().requires_grad_(True))
    return out


# ---- encoder ---------------------------------------------------------------------------------------------------------
# 32-node tiles, 4 per workgroup (matrix-core kernels); 256-thread blocks and 64-node chunks (valu kernels)
ENC_N = [1, 31, 32, 33, 127, 129, 257]
# "Wc" / "Wa": dense weights off a boundary with the tables aligned -- the matrix-core kernels stay (they read those per
# element)
ENC_PLACES = {"aligned": {}, "valu": {}, "Echg": {6: 4}, "Epdg": {7: 4}, "Epv": {8: 4}, "Wc": {0: 4}, "Wa": {4: 12},
              "all4": {i: 4 for i in range(9)}, "all8": {i: 8 for i in range(9)}, "all12": {i: 12 for i in range(9)}}


@functools.lru_cache(maxsize=None)
def _enc_case(N):
    x_cont, x_cat, g_h = pn.encoder_inputs(N, seed=N)
    params = pn.encoder_params()
    h_ref, leaves = pn.encoder_ref(x_cont, x_cat, params, g_h)
    return x_cont, x_cat, g_h, params, h_ref.detach(), [l.grad for l in leaves]


def _run_encoder(dev, monkeypatch, N, kind, g_offset=None):
    from deepmetv2_amd import dense
    x_cont, x_cat, g_h, params, _, _ = _enc_case(N)
    if kind == "valu":
        monkeypatch.setenv("DMET_ENCODER_FWD", "valu")
        monkeypatch.setenv("DMET_ENCODER_BWD", "valu")
    ps = _placed(params, dev, ENC_PLACES[kind])
    big = torch.cat([x_cont, x_cat.float()], dim=1).to(dev)          # strided view, as split_features hands over
    h = dense.encode(big[:, :8], x_cat.to(dev), *ps)
    g = g_h.to(dev)
    h.backward(g if g_offset is None else misaligned(g, g_offset))
    return h.detach(), [p.grad for p in ps]


def _check_encoder(N, h, grads):
    _, _, _, _, h_ref, g_ref = _enc_case(N)
    close(h, h_ref, "h")
    for n, g, r in zip(pn.ENCODER_PARAM_NAMES, grads, g_ref):
        close(g, r, "grad", n)


@pytest.mark.parametrize("kind", list(ENC_PLACES))
@pytest.mark.parametrize("N", ENC_N)
def test_encoder_routes_match_reference(dev, monkeypatch, N, kind):
    """dense.encode forward and backward: default route, both valu switches, each embedding table unaligned alone (one
    case per term of the dispatch condition), all nine parameters at 4, 8 and 12 bytes past a boundary."""
    h, grads = _run_encoder(dev, monkeypatch, N, kind)
    _check_encoder(N, h, grads)


@pytest.mark.parametrize("kind", ["Echg", "Epdg", "Epv", "all4", "all8", "all12"])
@pytest.mark.parametrize("N", ENC_N)
def test_encoder_unaligned_table_takes_the_valu_kernels(dev, monkeypatch, N, kind):
    """An unaligned table sends both directions to the scalar-weight kernels: same kernel, same grid, same values as
    under DMET_ENCODER_FWD/BWD=valu, hence the same bits."""
    _default_route_only("DMET_ENCODER_FWD", "DMET_ENCODER_BWD")
    h_u, g_u = _run_encoder(dev, monkeypatch, N, kind)
    h_v, g_v = _run_encoder(dev, monkeypatch, N, "valu")
    _equal(h_u, h_v, "h")
    for n, a, b in zip(pn.ENCODER_PARAM_NAMES, g_u, g_v):
        _equal(a, b, n)


@pytest.mark.parametrize("kind", ["Wc", "Wa"])
@pytest.mark.parametrize("N", [33, 257])
def test_encoder_unaligned_dense_weight_is_not_in_the_dispatch(dev, monkeypatch, N, kind):
    """Only the tables are in the dispatch condition: an unaligned Wc or Wa keeps the route and the bits of the aligned call."""
    h0, g0 = _run_encoder(dev, monkeypatch, N, "aligned")
    h1, g1 = _run_encoder(dev, monkeypatch, N, kind)
    _equal(h1, h0, "h")
    for n, a, b in zip(pn.ENCODER_PARAM_NAMES, g1, g0):
        _equal(a, b, n)


def test_encoder_one_workgroup_walks_all_tiles(dev, monkeypatch):
    """DMET_ENC_GRID=1 at N = 257: one workgroup (four wavefronts) walks the nine 32-node tiles, the last with one node, and
    its three-stage prefetch runs dry at different iterations per wavefront: same bits as one tile per wavefront."""
    monkeypatch.delenv("DMET_ENC_GRID", raising=False)
    h0, g0 = _run_encoder(dev, monkeypatch, 257, "aligned")
    monkeypatch.setenv("DMET_ENC_GRID", "1")
    h1, g1 = _run_encoder(dev, monkeypatch, 257, "aligned")
    _equal(h1, h0, "h")
    _check_encoder(257, h1, g1)


@pytest.mark.parametrize("N", [33, 257])
def test_encoder_backward_takes_an_unaligned_upstream_gradient(dev, monkeypatch, N):
    h0, g0 = _run_encoder(dev, monkeypatch, N, "aligned")
    h1, g1 = _run_encoder(dev, monkeypatch, N, "aligned", g_offset=4)
    _check_encoder(N, h1, g1)
    for n, a, b in zip(pn.ENCODER_PARAM_NAMES, g1, g0):
        _equal(a, b, n)


# ---- head ------------------------------------------------------------------------------------------------------------
HEAD_N = [1, 63, 64, 65, 255, 257]          # 64-node wave chunks, 256 nodes per workgroup
HEAD_PLACES = {"aligned": {}, "valu": {}, "W1": {1: 4}, "b1": {2: 4}, "W2": {3: 4},
               "all4": {i: 4 for i in range(1, 5)}, "all8": {i: 8 for i in range(1, 5)},
               "all12": {i: 12 for i in range(1, 5)}}
HEAD_NAMES = ["emb", "W1", "b1", "W2", "b2"]


@functools.lru_cache(maxsize=None)
def _head_case(N):
    emb, g_out = pn.head_inputs(N, seed=N)
    hp = pn.head_params()
    out, leaves = pn.head_ref(emb, *hp, g_out)
    return emb, g_out, hp, out.detach(), [l.grad for l in leaves]


def _run_head(dev, monkeypatch, N, where, valu=(), g_offset=None):
    """where: {index into (emb, W1, b1, W2, b2): byte offset}; valu: the directions switched to the scalar-weight kernel;
    g_offset: where the upstream gradient sits."""
    from deepmetv2_amd import dense
    emb, g_out, hp, _, _ = _head_case(N)
    for d in valu:
        monkeypatch.setenv(f"DMET_HEAD_{d}", "valu")
    ts = _placed([emb] + hp, dev, where)
    out = dense.head(*ts)
    g = g_out.to(dev)
    out.backward(g if g_offset is None else misaligned(g, g_offset))
    return out.detach(), [t.grad for t in ts]


def _check_head(N, out, grads):
    _, _, _, out_ref, g_ref = _head_case(N)
    close(out, out_ref, "head")
    for n, g, r in zip(HEAD_NAMES, grads, g_ref):
        close(g, r, "grad", n)


@pytest.mark.parametrize("kind", list(HEAD_PLACES))
@pytest.mark.parametrize("N", HEAD_N)
def test_head_routes_match_reference(dev, monkeypatch, N, kind):
    """dense.head forward and backward (g_emb and the four parameter gradients): default route, both valu switches,
    each of W1, b1, W2 unaligned alone, all four parameters unaligned."""
    out, grads = _run_head(dev, monkeypatch, N, HEAD_PLACES[kind], valu=("FWD", "BWD") if kind == "valu" else ())
    _check_head(N, out, grads)


@pytest.mark.parametrize("N", HEAD_N)
def test_head_unaligned_b2_is_not_in_the_dispatch(dev, monkeypatch, N):
    """b2 is read as one scalar by every kernel: wherever it sits, the route and the bits are the aligned call's."""
    out0, g0 = _run_head(dev, monkeypatch, N, {})
    out1, g1 = _run_head(dev, monkeypatch, N, {4: 4})
    _check_head(N, out1, g1)
    _equal(out1, out0, "out")
    for n, a, b in zip(HEAD_NAMES, g1, g0):
        _equal(a, b, n)


@pytest.mark.parametrize("kind", ["W1", "b1", "W2"])
@pytest.mark.parametrize("N", HEAD_N)
def test_head_unaligned_parameter_takes_the_valu_forward(dev, monkeypatch, N, kind):
    """W1, b1 or W2 off a boundary sends the forward to the scalar-weight kernel (the backward kernel reads them element by
    element and stays): the bits of DMET_HEAD_FWD=valu."""
    _default_route_only("DMET_HEAD_FWD", "DMET_HEAD_BWD")
    out_u, g_u = _run_head(dev, monkeypatch, N, HEAD_PLACES[kind])
    out_v, g_v = _run_head(dev, monkeypatch, N, {}, valu=("FWD",))
    _equal(out_u, out_v, "out")
    for n, a, b in zip(HEAD_NAMES, g_u, g_v):
        _equal(a, b, n)


@pytest.mark.parametrize("offset", [4, 8, 12])
@pytest.mark.parametrize("N", [1, 65, 257])
def test_head_takes_an_unaligned_emb(dev, monkeypatch, N, offset):
    """A contiguous emb that starts off a boundary (a row range of a larger buffer): the reference, and the aligned bits."""
    out0, g0 = _run_head(dev, monkeypatch, N, {})
    out1, g1 = _run_head(dev, monkeypatch, N, {0: offset})
    _check_head(N, out1, g1)
    _equal(out1, out0, "out")
    for n, a, b in zip(HEAD_NAMES, g1, g0):
        _equal(a, b, n)


@pytest.mark.parametrize("valu", [(), ("FWD", "BWD")], ids=["default", "valu"])
@pytest.mark.parametrize("N", [1, 65, 257])
def test_head_backward_takes_an_unaligned_upstream_gradient(dev, monkeypatch, N, valu):
    """g_out (and emb with it) off a boundary, through either backward kernel: the reference, and the aligned bits."""
    out0, g0 = _run_head(dev, monkeypatch, N, {}, valu=valu)
    out1, g1 = _run_head(dev, monkeypatch, N, {0: 8}, valu=valu, g_offset=4)
    _check_head(N, out1, g1)
    for n, a, b in zip(HEAD_NAMES, g1, g0):
        _equal(a, b, n)


# ---- BatchNorm into the head (dmet_bn_head_fwd_f32) -------------------------------------------------------------------
BNH_N = [2, 63, 65, 257]
EPS, MOMENTUM = 1e-5, 0.1       # torch.nn.BatchNorm1d's defaults
# index into (gamma, beta, W1, b1, W2, b2) -> byte offset; "valu": DMET_HEAD_FWD=valu
BNH_DECLINED = {"gamma": {0: 4}, "beta": {1: 8}, "W1": {2: 4}, "b1": {3: 12}, "W2": {4: 4}, "valu": {}}


@functools.lru_cache(maxsize=None)
def _bnh_case(N, with_res):
    raw, res, _ = pn.bn_rows(N, 32, seed=N + 32)
    res = res if with_res else None
    state, hp = pn.bn_state(32, seed=32), pn.head_params()
    g_out = torch.randn(N, generator=torch.Generator().manual_seed(N))
    out, emb, ref, x64, r64, leaves = pn.bn_head_ref(raw, state, True, res, hp, g_out)
    return raw, res, state, hp, g_out, out.detach(), emb.detach(), ref, x64, r64, leaves


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("N", BNH_N)
def test_bn_head_fwd_accepts_aligned_operands(dev, N, with_res):
    """_native.bn_head_fwd with everything aligned returns (emb, out): emb has the bits of bn_apply, out the bits of
    head_fwd on that emb, and both meet their references (statistics from bn_stats, running statistics included).
    Under DMET_HEAD_FWD=valu the entry declines by design: the two separate steps are held to the references instead."""
    from deepmetv2_amd import _native
    raw, res, state, hp, _, out_ref, emb_ref, ref, _, _, _ = _bnh_case(N, with_res)
    raw_d, res_d = raw.to(dev), (res.to(dev) if with_res else None)
    gamma, beta = state["weight"].to(dev), state["bias"].to(dev)
    rm, rv = state["running_mean"].to(dev), state["running_var"].to(dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    hp_d = [t.to(dev) for t in hp]
    mean, invstd = _native.bn_stats(raw_d, EPS, MOMENTUM, rm, rv, nbt)
    got = _native.bn_head_fwd(raw_d, res_d, gamma, beta, mean, invstd, hp_d)
    emb2 = _native.bn_apply(raw_d, res_d, gamma, beta, mean, invstd)
    if os.environ.get("DMET_HEAD_FWD") == "valu":
        assert got is None
        emb, out = emb2, _native.head_fwd(emb2, hp_d)
    else:
        assert got is not None, "dmet_bn_head_fwd_f32 declined aligned operands"
        emb, out = got
        _equal(emb, emb2, "emb")
        _equal(out, _native.head_fwd(emb, hp_d), "out")
    close(emb, emb_ref, "bn_y")
    close(out, out_ref, "head")
    close(rm, ref.running_mean, "running", "running_mean")
    close(rv, ref.running_var, "running", "running_var")
    assert int(nbt) == int(ref.num_batches_tracked) == 1


@pytest.mark.parametrize("kind", ["aligned"] + list(BNH_DECLINED))
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("N", BNH_N)
def test_batch_norm_into_head_matches_reference(dev, monkeypatch, N, with_res, kind):
    """dense.batch_norm(raw, bn, residual, next_build=head_prebuild_hook(...)) then dense.head(...): output and every
    gradient (raw, residual, BatchNorm's, the head's) against the reference.  With gamma, beta, W1, b1 or W2 unaligned,
    or under DMET_HEAD_FWD=valu, dmet_bn_head_fwd_f32 declines: _native.bn_head_fwd returns None, nothing is left in
    dense._HEAD_PREBUILT and Python runs bn_apply and the head's own forward."""
    from deepmetv2_amd import _native, dense
    raw, res, state, hp, g_out, out_ref, emb_ref, ref, x64, r64, leaves = _bnh_case(N, with_res)
    monkeypatch.setattr(dense, "HEAD_FUSE", "1")
    where = BNH_DECLINED.get(kind, {})
    if kind == "valu":
        monkeypatch.setenv("DMET_HEAD_FWD", "valu")
    bn = pn.bn_module(state, True).to(dev)
    if 0 in where:
        bn.weight.data = misaligned(bn.weight.data, where[0])
    if 1 in where:
        bn.bias.data = misaligned(bn.bias.data, where[1])
    hp_d = _placed(hp, dev, {i - 2: o for i, o in where.items() if i >= 2})
    raw_d = raw.to(dev).requires_grad_(True)
    res_d = res.to(dev).requires_grad_(True) if with_res else None
    seen = _spy(monkeypatch, _native, "bn_head_fwd")
    dense._HEAD_PREBUILT[0] = None
    emb = dense.batch_norm(raw_d, bn, res_d, next_build=dense.head_prebuild_hook(*hp_d))
    assert len(seen) == 1
    if kind != "aligned":
        assert seen[0] is None, f"{kind}: dmet_bn_head_fwd_f32 launched"
        assert dense._HEAD_PREBUILT[0] is None
    emb.retain_grad()
    out = dense.head(emb, *hp_d)
    assert dense._HEAD_PREBUILT[0] is None
    out.backward(g_out.to(dev))
    close(emb, emb_ref, "bn_y")
    close(out, out_ref, "head")
    close(raw_d.grad, x64.grad, "g_x", "raw")
    close(emb.grad, leaves[0].grad, "grad", "emb")
    if with_res:
        close(res_d.grad, r64.grad, "grad", "residual")
        _equal(res_d.grad, emb.grad, "residual")
    close(bn.weight.grad, ref.weight.grad, "grad", "bn.weight")
    close(bn.bias.grad, ref.bias.grad, "grad", "bn.bias")
    for n, t, l in zip(HEAD_NAMES[1:], hp_d, leaves[1:]):
        close(t.grad, l.grad, "grad", n)
    close(bn.running_mean, ref.running_mean, "running", "running_mean")
    close(bn.running_var, ref.running_var, "running", "running_var")
    assert int(bn.num_batches_tracked) == 1


def test_prebuilt_pair_serves_its_own_emb_only(dev, monkeypatch):
    """After an accepted prebuild, dense.head on another tensor of the same shape computes that tensor's own result and
    the pair is dropped, not kept for later."""
    from deepmetv2_amd import _native, dense
    _default_route_only("DMET_HEAD_FWD")
    N = 65
    raw, _, state, hp, _, _, _, _, _, _, _ = _bnh_case(N, False)
    monkeypatch.setattr(dense, "HEAD_FUSE", "1")
    bn = pn.bn_module(state, True).to(dev)
    hp_d = [t.to(dev) for t in hp]
    dense._HEAD_PREBUILT[0] = None
    with torch.no_grad():
        emb = dense.batch_norm(raw.to(dev), bn, None, next_build=dense.head_prebuild_hook(*hp_d))
        pre = dense._HEAD_PREBUILT[0]
        assert pre is not None and pre[0].data_ptr() == emb.data_ptr()
        other_cpu, _ = pn.head_inputs(N, seed=1234)
        other = other_cpu.to(dev)
        out_other = dense.head(other, *hp_d)
        assert dense._HEAD_PREBUILT[0] is None
        _equal(out_other, _native.head_fwd(other, hp_d), "out of the other emb")
        close(out_other, pn.head_ref(other_cpu, *hp)[0], "head")
        assert not torch.equal(out_other, pre[1])
        _equal(dense.head(emb, *hp_d), pre[1], "out of the BatchNorm's emb, computed afresh")


# ---- encoder + BatchNorm as one node (dmet_encode_bn_bwd_f32) ---------------------------------------------------------
EBN_N = sorted(pn.ENCODE_BN_SEEDS)      # 2, 33, 129, 257


@functools.lru_cache(maxsize=None)
def _ebn_case(N):
    x_cont, x_cat, g_y = pn.encoder_inputs(N, seed=pn.ENCODE_BN_SEEDS[N])
    params, state = pn.encoder_params(), pn.bn_state(32, seed=32)
    y, leaves, ref = pn.encode_bn_ref(x_cont, x_cat, params, state, g_y)
    return x_cont, x_cat, g_y, params, state, y.detach(), [l.grad for l in leaves], ref


def _run_encode_bn(dev, monkeypatch, N, kind, fuse="1", g_offset=None):
    from deepmetv2_amd import _native, dense
    x_cont, x_cat, g_y, params, state, _, _, _ = _ebn_case(N)
    monkeypatch.setattr(dense, "ENC_BN_FUSE", fuse)
    if kind == "valu_bwd":
        monkeypatch.setenv("DMET_ENCODER_BWD", "valu")
    bn = pn.bn_module(state, True).to(dev)
    if kind == "bn_weight":
        bn.weight.data = misaligned(bn.weight.data, 4)
    ps = _placed(params, dev, {7: 8} if kind == "table" else {})
    seen = _spy(monkeypatch, _native, "encode_bn_bwd")
    big = torch.cat([x_cont, x_cat.float()], dim=1).to(dev)
    y = dense.encode_bn(big[:, :8], x_cat.to(dev), bn, None, *ps)
    g = g_y.to(dev)
    y.backward(g if g_offset is None else misaligned(g, g_offset))
    return y.detach(), [p.grad for p in ps], bn, seen


def _check_encode_bn(N, y, grads, bn):
    _, _, _, _, _, y_ref, g_ref, ref = _ebn_case(N)
    close(y, y_ref, "bn_y")
    for n, g, r in zip(pn.ENCODER_PARAM_NAMES, grads, g_ref):
        close(g, r, "grad", n)
    close(bn.weight.grad, ref.weight.grad, "grad", "bn.weight")
    close(bn.bias.grad, ref.bias.grad, "grad", "bn.bias")
    close(bn.running_mean, ref.running_mean, "running", "running_mean")
    close(bn.running_var, ref.running_var, "running", "running_var")
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1


@pytest.mark.parametrize("kind", ["aligned", "table", "bn_weight", "valu_bwd"])
@pytest.mark.parametrize("N", EBN_N)
def test_encode_bn_matches_reference(dev, monkeypatch, N, kind):
    """dense.encode_bn with a training-mode BatchNorm1d(32) and next_build=None against encode_bn_ref: output, nine
    encoder gradients, the BatchNorm's, the running statistics.  With one table or bn.weight unaligned, or under
    DMET_ENCODER_BWD=valu, _native.encode_bn_bwd returns None and _EncodeBN.backward runs bn_bwd and encode_bwd."""
    y, grads, bn, seen = _run_encode_bn(dev, monkeypatch, N, kind)
    assert len(seen) == 1
    if kind != "aligned":
        assert seen[0] is None, f"{kind}: the fused backward ran"
    _check_encode_bn(N, y, grads, bn)


@pytest.mark.parametrize("N", [33, 257])
def test_encode_bn_backward_takes_an_unaligned_upstream_gradient(dev, monkeypatch, N):
    """g_y off a boundary: _native.encode_bn_bwd returns None before its statistics launch (whose entry requires g_y
    aligned) and the two separate steps copy it -- the reference, and the bits of the aligned call."""
    y0, g0, bn0, _ = _run_encode_bn(dev, monkeypatch, N, "aligned")
    y1, g1, bn1, seen = _run_encode_bn(dev, monkeypatch, N, "aligned", g_offset=4)
    assert len(seen) == 1 and seen[0] is None
    _check_encode_bn(N, y1, g1, bn1)
    for n, a, b in zip(pn.ENCODER_PARAM_NAMES, g1, g0):
        _equal(a, b, n)
    _equal(bn1.weight.grad, bn0.weight.grad, "bn.weight")
    _equal(bn1.bias.grad, bn0.bias.grad, "bn.bias")


@pytest.mark.parametrize("N", EBN_N)
def test_encode_bn_fused_backward_has_the_bits_of_the_two_steps(dev, monkeypatch, N):
    """Aligned operands: _native.encode_bn_bwd returns a result, and the whole node has the bits of ENC_BN_FUSE = "0"
    (batch_norm(encode(...))) at the tile edges too."""
    _default_route_only("DMET_ENCODER_BWD")
    y1, g1, bn1, seen = _run_encode_bn(dev, monkeypatch, N, "aligned", fuse="1")
    assert len(seen) == 1 and seen[0] is not None, "dmet_encode_bn_bwd_f32 declined aligned operands"
    y0, g0, bn0, seen0 = _run_encode_bn(dev, monkeypatch, N, "aligned", fuse="0")
    assert not seen0
    _equal(y1, y0, "y")
    for n, a, b in zip(pn.ENCODER_PARAM_NAMES, g1, g0):
        _equal(a, b, n)
    _equal(bn1.weight.grad, bn0.weight.grad, "bn.weight")
    _equal(bn1.bias.grad, bn0.bias.grad, "bn.bias")
    _equal(bn1.running_mean, bn0.running_mean, "running_mean")
    _equal(bn1.running_var, bn0.running_var, "running_var")


# ---- BatchNorm on unaligned vectors -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_case(N, H, training, with_res):
    x, r, g_y = pn.bn_rows(N, H, seed=N + H)
    r = r if with_res else None
    state = pn.bn_state(H, seed=H)
    y, ref, x64, r64 = pn.bn_ref(x, state, training, r, g_y)
    return x, r, g_y, state, y.detach(), ref, x64.grad, (r64.grad if with_res else None)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N,H", [(2, 4), (3, 8), (257, 32), (1025, 64)])
def test_batch_norm_takes_unaligned_operands(dev, N, H, training, with_res):
    """dense.batch_norm with bn.weight / bn.bias re-homed to unaligned views, with an unaligned contiguous x (and residual),
    and with an unaligned upstream gradient: the reference each time, and the bits of the aligned call."""
    from deepmetv2_amd import dense
    x, r, g_y, state, y_ref, ref, gx_ref, gr_ref = _bn_case(N, H, training, with_res)
    runs = {}
    for place in ("aligned", "params", "rows", "grad"):
        bn = pn.bn_module(state, training).to(dev)
        if place == "params":
            bn.weight.data = misaligned(bn.weight.data, 4)
            bn.bias.data = misaligned(bn.bias.data, 12)
        xd, rd, gd = x.to(dev), (r.to(dev) if with_res else None), g_y.to(dev)
        if place == "rows":
            xd, rd = misaligned(xd, 8), (misaligned(rd, 4) if with_res else None)
        if place == "grad":
            gd = misaligned(gd, 4)
        xd = xd.detach().requires_grad_(True)
        rd = rd.detach().requires_grad_(True) if with_res else None
        y = dense.batch_norm(xd, bn, residual=rd)
        y.backward(gd)
        close(y, y_ref, "bn_y", f"{place}: y")
        close(xd.grad, gx_ref, "g_x", f"{place}: g_x")
        if with_res:
            assert torch.equal(rd.grad.cpu(), g_y), f"{place}: residual gradient"
        close(bn.weight.grad, ref.weight.grad, "grad", f"{place}: bn.weight")
        close(bn.bias.grad, ref.bias.grad, "grad", f"{place}: bn.bias")
        close(bn.running_mean, ref.running_mean, "running", f"{place}: running_mean")
        close(bn.running_var, ref.running_var, "running", f"{place}: running_var")
        assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)
        runs[place] = (y.detach(), xd.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)
    for place in ("params", "rows", "grad"):
        for n, a, b in zip(("y", "g_x", "bn.weight", "bn.bias", "running_mean", "running_var"), runs[place], runs["aligned"]):
            _equal(a, b, f"{place}: {n}")

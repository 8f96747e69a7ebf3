"""The helpers of tests/per_node_reference.py against stock torch on the CPU: `misaligned` gives the offsets asked for,
and the float64 references agree with the float32 modules they restate (bars of tests/test_gpu_parity.py for the same
quantities)."""
import pytest
import torch

import per_node_reference as pn
from oracle import ref_model


@pytest.mark.parametrize("byte_offset", [4, 8, 12])
@pytest.mark.parametrize("shape", [(1,), (16,), (3, 8), (16, 32), (257, 32)])
def test_misaligned_gives_the_offset_and_keeps_it(shape, byte_offset):
    t = torch.randn(*shape)
    m = pn.misaligned(t, byte_offset)
    assert m.data_ptr() % 16 == byte_offset
    assert m.shape == t.shape and m.dtype == t.dtype and m.device == t.device and m.is_contiguous()
    assert torch.equal(m, t)
    leaf = m.detach().requires_grad_(True)
    assert leaf.data_ptr() % 16 == byte_offset and leaf.is_leaf
    # what a module does with it: a Parameter re-homed onto the view keeps the place
    bn = torch.nn.BatchNorm1d(4)
    bn.weight.data = pn.misaligned(bn.weight.data, byte_offset)
    assert bn.weight.data_ptr() % 16 == byte_offset and bn.weight.detach().data_ptr() % 16 == byte_offset


def test_misaligned_default_and_bad_offsets():
    assert pn.misaligned(torch.zeros(5)).data_ptr() % 16 == 4
    for bad in (0, 2, 16):
        with pytest.raises(ValueError):
            pn.misaligned(torch.zeros(5), bad)
    with pytest.raises(ValueError):
        pn.misaligned(torch.zeros(5, dtype=torch.float64), 4)
    assert pn.misaligned(torch.zeros(5, dtype=torch.float64), 8).data_ptr() % 16 == 8


@pytest.mark.parametrize("N", [1, 33, 257])
def test_encoder_ref_agrees_with_the_oracle_model(N):
    x_cont, x_cat, g_h = pn.encoder_inputs(N, seed=N)
    assert set(x_cat[:, 0].tolist()) <= set(pn.PDG_POOL)
    torch.manual_seed(11)
    model = ref_model.RefGraphMETNetwork(8, 3, output_dim=1, hidden_dim=32, conv_depth=1)
    params = pn.encoder_params(seed=11)
    sd = dict(model.named_parameters())
    for n, p in zip(pn.ENCODER_PARAM_NAMES, params):
        assert torch.equal(p, sd[n].detach())
    model.bn_all = torch.nn.Identity()          # node_embedding() = the encoder, then bn_all
    h32 = model.node_embedding(x_cont, x_cat).detach()
    h, leaves = pn.encoder_ref(x_cont, x_cat, params, g_h)
    assert h.dtype == torch.float64
    torch.testing.assert_close(h32.double(), h.detach(), rtol=1e-5, atol=1e-5)
    # the same modules in float64 give encoder_ref's bits, forward and backward: one reference, two spellings
    m64 = model.double()
    h64 = m64.node_embedding(x_cont.double(), x_cat)
    h64.backward(g_h.double())
    assert torch.equal(h64.detach(), h.detach())
    sd = dict(m64.named_parameters())
    for n, leaf in zip(pn.ENCODER_PARAM_NAMES, leaves):
        assert torch.equal(sd[n].grad, leaf.grad), n


def test_encoder_ref_unknown_pdg_ids_keep_their_value_as_class():
    params = pn.encoder_params()
    x_cont = torch.zeros(4, 8)
    x_cat = torch.tensor([[5, 0, 0], [130, 0, 0], [3, 0, 0], [13, 0, 0]])    # 130 -> class 5, 13 -> class 3
    h, _ = pn.encoder_ref(x_cont, x_cat, params)
    assert torch.equal(h[0], h[1]) and torch.equal(h[2], h[3]) and not torch.equal(h[0], h[2])


@pytest.mark.parametrize("N", [1, 65, 257])
def test_head_ref_agrees_with_float32_torch(N):
    g = torch.Generator().manual_seed(N)
    emb = torch.randn(N, 32, generator=g)
    W1, b1 = torch.randn(16, 32, generator=g) * 0.3, torch.randn(16, generator=g) * 0.3
    W2, b2 = torch.randn(1, 16, generator=g) * 0.5, torch.randn(1, generator=g)
    gup = torch.randn(N, generator=g)
    out, leaves = pn.head_ref(emb, W1, b1, W2, b2, gup)
    net = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.ELU(), torch.nn.Linear(16, 1))
    with torch.no_grad():
        net[0].weight.copy_(W1); net[0].bias.copy_(b1); net[2].weight.copy_(W2); net[2].bias.copy_(b2)
    e32 = emb.clone().requires_grad_(True)
    o32 = net(e32).squeeze(-1).sigmoid()
    o32.backward(gup)
    torch.testing.assert_close(o32.detach().double(), out.detach(), rtol=1e-5, atol=1e-6)
    for got, leaf in zip([e32, net[0].weight, net[0].bias, net[2].weight, net[2].bias], leaves):
        r = leaf.grad
        torch.testing.assert_close(got.grad.double(), r, rtol=1e-4, atol=1e-5 * max(1.0, float(r.abs().max())))


@pytest.mark.parametrize("N,H,residual,training", [(3, 8, True, True), (257, 32, False, True), (257, 32, True, False),
                                                   (1025, 64, True, True)])
def test_bn_ref_agrees_with_float32_torch(N, H, residual, training):
    g = torch.Generator().manual_seed(N + H)
    x = torch.randn(N, H, generator=g) * 0.7 + 3.0
    r = torch.randn(N, H, generator=g) if residual else None
    gup = torch.randn(N, H, generator=g)
    state = pn.bn_state(H, seed=H)
    y, ref, x64, r64 = pn.bn_ref(x, state, training, r, gup)
    bn = pn.bn_module(state, training)
    x32 = x.clone().requires_grad_(True)
    y32 = bn(x32) + (r if residual else 0.0)
    y32.backward(gup)
    torch.testing.assert_close(y32.detach().double(), y.detach(), rtol=2e-5, atol=2e-5)
    gs = float(x64.grad.abs().max())
    torch.testing.assert_close(x32.grad.double(), x64.grad, rtol=1e-4, atol=2e-5 * max(gs, 1.0))
    if residual:
        assert torch.equal(r64.grad, gup.double())
    for a, b in ((bn.weight.grad, ref.weight.grad), (bn.bias.grad, ref.bias.grad)):
        torch.testing.assert_close(a.double(), b, rtol=1e-4, atol=1e-5 * max(1.0, float(b.abs().max())))
    torch.testing.assert_close(bn.running_mean.double(), ref.running_mean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(bn.running_var.double(), ref.running_var, rtol=1e-5, atol=1e-5)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == (1 if training else 0)


def test_encode_bn_ref_is_the_composition():
    x_cont, x_cat, _ = pn.encoder_inputs(33, seed=33)
    params = pn.encoder_params()
    state = pn.bn_state(32, seed=5)
    g_y = torch.randn(33, 32, generator=torch.Generator().manual_seed(1))
    y, leaves, ref = pn.encode_bn_ref(x_cont, x_cat, params, state, g_y)
    h, leaves2 = pn.encoder_ref(x_cont, x_cat, params)
    y2, ref2, h_leaf, _ = pn.bn_ref(h.detach(), state, True, None, g_y)
    assert torch.equal(y.detach(), y2.detach())
    h.backward(h_leaf.grad)
    for a, b in zip(leaves, leaves2):
        assert torch.equal(a.grad, b.grad)
    assert torch.equal(ref.weight.grad, ref2.weight.grad) and torch.equal(ref.running_var, ref2.running_var)
    assert int(ref.num_batches_tracked) == 1


# ---- the small-batch inputs of tests/test_gpu_per_node_routes.py are well conditioned -------------------------------
# (per_node_reference's docstring, "Inputs"): stock float32 torch on the CPU stays within a quarter of every bar on them,
# so a kernel that misses a bar there is wrong, not unlucky.
_MARGIN = 0.25


def _encode_bn_float32_ratios(N, seed):
    x_cont, x_cat, g_y = pn.encoder_inputs(N, seed=seed)
    params, state = pn.encoder_params(), pn.bn_state(32, seed=32)
    y, leaves, ref = pn.encode_bn_ref(x_cont, x_cat, params, state, g_y)
    y32, leaves32, ref32 = pn.encode_bn_ref(x_cont, x_cat, params, state, g_y, dtype=torch.float32)
    worst = [pn.bar_ratio(y32, y, "bn_y"), pn.bar_ratio(ref32.weight.grad, ref.weight.grad, "grad"),
             pn.bar_ratio(ref32.bias.grad, ref.bias.grad, "grad")]
    return worst + [pn.bar_ratio(a.grad, b.grad, "grad") for a, b in zip(leaves32, leaves)]


@pytest.mark.parametrize("N", sorted(pn.ENCODE_BN_SEEDS))
def test_encode_bn_inputs_leave_float32_a_margin(N):
    worst = _encode_bn_float32_ratios(N, pn.ENCODE_BN_SEEDS[N])
    assert max(worst) <= _MARGIN, worst


def test_a_random_two_node_batch_is_ill_conditioned():
    """Why ENCODE_BN_SEEDS[2] is not simply 2: on that two-node batch stock float32 torch itself misses a gradient bar."""
    assert max(_encode_bn_float32_ratios(2, 2)) > 1.0


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("N,H", [(2, 4), (3, 8), (2, 32)])
def test_small_batch_rows_leave_float32_a_margin(N, H, with_res):
    x, r, g_y = pn.bn_rows(N, H, seed=N + H)
    assert float(x.double().var(0, unbiased=False).min()) >= 1.0 / 16
    state = pn.bn_state(H, seed=H)
    y, ref, x64, _ = pn.bn_ref(x, state, True, r if with_res else None, g_y)
    y32, ref32, x32, _ = pn.bn_ref(x, state, True, r if with_res else None, g_y, dtype=torch.float32)
    worst = [pn.bar_ratio(y32, y, "bn_y"), pn.bar_ratio(x32.grad, x64.grad, "g_x"),
             pn.bar_ratio(ref32.weight.grad, ref.weight.grad, "grad"), pn.bar_ratio(ref32.bias.grad, ref.bias.grad, "grad")]
    assert max(worst) <= _MARGIN, worst
    if H != 32:
        return
    hp = pn.head_params()
    g_out = torch.randn(N, generator=torch.Generator().manual_seed(N))
    out, emb, ref, x64, r64, leaves = pn.bn_head_ref(x, state, True, r if with_res else None, hp, g_out)
    out32, emb32, ref32, x32, r32, leaves32 = pn.bn_head_ref(x, state, True, r if with_res else None, hp, g_out,
                                                             dtype=torch.float32)
    worst = [pn.bar_ratio(out32, out, "head"), pn.bar_ratio(emb32, emb, "bn_y"), pn.bar_ratio(x32.grad, x64.grad, "g_x"),
             pn.bar_ratio(ref32.weight.grad, ref.weight.grad, "grad"), pn.bar_ratio(ref32.bias.grad, ref.bias.grad, "grad")]
    worst += [pn.bar_ratio(a.grad, b.grad, "grad") for a, b in zip(leaves32, leaves)]
    assert max(worst) <= _MARGIN, worst

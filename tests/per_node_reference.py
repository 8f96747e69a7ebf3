"""Float64 CPU references with backward for the per-node chain (encoder, BatchNorm, head and their compositions), and
`misaligned`, which puts a tensor where the kernels' 16-byte dispatch conditions do not hold.  Helpers for
test_per_node_reference_host.py and test_gpu_per_node_routes.py; nothing here is collected as a test.

Every reference takes float32 (or float64) CPU tensors, computes in float64 with plain torch operators and, when an
upstream gradient is given, runs backward; the float64 leaves it returns carry the reference gradients in `.grad`.
(`dtype=torch.float32` runs the same operators in float32: what stock torch gives, for the host tests.)

The bars are the ones tests/test_gpu_parity.py uses for the same quantities; `close` applies them by name.

Inputs.  The bars were set on batches of thousands of rows.  BatchNorm over two or three rows is as well conditioned
as the rows are apart: its backward forms gamma * invstd * (g - mean_g - xhat * mean_gx), a difference of terms that
cancel to eps / (var + eps) of their size at N = 2, so float32 rounding in xhat comes out multiplied by invstd.  On a
random two-node encoder batch some of the 32 channels nearly coincide (both saturated by the ELU) and stock float32
torch on the CPU itself can miss the gradient bars (encoder_inputs(2, seed=2) does, by a factor of two: the host test
test_a_random_two_node_batch_is_ill_conditioned keeps that on record).  The small batches here are therefore chosen on
the reference alone: `bn_rows` spreads a handful of rows at least 0.5 apart in every channel,
and ENCODE_BN_SEEDS[2] is a two-node batch on which stock float32 torch stays within a quarter of every bar
(test_per_node_reference_host.py asserts that margin for every small-batch input of the GPU tests).
"""
import torch

from oracle import ref_model

F = torch.nn.functional

# the order of dense.encode's parameters (Wc, bc, Wk, bk, Wa, ba, Echg, Epdg, Epv) as names of the reference model
ENCODER_PARAM_NAMES = ["embed_continuous.0.weight", "embed_continuous.0.bias", "embed_categorical.0.weight",
                       "embed_categorical.0.bias", "encode_all.0.weight", "encode_all.0.bias", "embed_charge.weight",
                       "embed_pdgid.weight", "embed_pv.weight"]
# ids of the reference's table and their negatives, plus 0 / 5 / 4 / 3, which are not in the table
PDG_POOL = (1, 2, 11, -11, 13, -13, 22, 130, 211, -211, 0, 5, 4, 3)


def misaligned(t: torch.Tensor, byte_offset: int = 4) -> torch.Tensor:
    """A contiguous tensor with the values, shape, device and dtype of `t` whose data_ptr() % 16 == byte_offset
    (4, 8 or 12): a view carved out of a buffer a few elements larger, as a parameter is that lives in somebody's flat
    buffer without padding.  The offset survives detach().requires_grad_(True); both are asserted here."""
    if byte_offset not in (4, 8, 12):
        raise ValueError(f"misaligned: byte_offset must be 4, 8 or 12, got {byte_offset}")
    es = t.element_size()
    if not t.is_floating_point() or byte_offset % es:
        raise ValueError(f"misaligned: a {t.dtype} tensor cannot start at byte offset {byte_offset} and carry a gradient")
    n = t.numel()
    buf = torch.empty(n + 16 // es + 1, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % es == 0
    first = ((byte_offset - buf.data_ptr()) % 16) // es
    out = buf[first:first + n].view(t.shape)
    out.copy_(t.detach())
    assert out.is_contiguous() and out.data_ptr() % 16 == byte_offset, (out.data_ptr() % 16, byte_offset)
    assert out.detach().requires_grad_(True).data_ptr() == out.data_ptr()
    return out


# name -> (rtol, atol); "grad" and "g_x" scale their atol with the reference (see `bar`)
BARS = {"h": (1e-5, 1e-5), "head": (1e-5, 1e-6), "bn_y": (2e-5, 2e-5), "running": (1e-5, 1e-5)}

# encoder_inputs seed per N for the encode_bn cases (N = 2: see "Inputs" above)
ENCODE_BN_SEEDS = {2: 172, 33: 33, 129: 129, 257: 257}


def bar(kind: str, ref: torch.Tensor):
    """(rtol, atol) of tests/test_gpu_parity.py for a quantity of this kind with reference `ref`: "h" encoder output,
    "head" head output, "bn_y" BatchNorm output, "running" running statistics, "grad" parameter gradients (and the
    head's g_emb), "g_x" BatchNorm's input gradient."""
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if kind == "grad":
        return 1e-4, 1e-5 * max(1.0, top)
    if kind == "g_x":
        return 1e-4, 2e-5 * max(top, 1.0)
    return BARS[kind]


def bar_ratio(got: torch.Tensor, ref: torch.Tensor, kind: str) -> float:
    """max |got - ref| / (atol + rtol |ref|): at most 1 when `got` meets the bar."""
    ref = ref.detach().double()
    rtol, atol = bar(kind, ref)
    if not ref.numel():
        return 0.0
    return float(((got.detach().cpu().double() - ref).abs() / (atol + rtol * ref.abs())).max())


def close(got: torch.Tensor, ref: torch.Tensor, kind: str, what: str = "") -> None:
    """assert_close of `got` (any device, float32) against the float64 reference at the bar of `kind`."""
    ref = ref.detach().double()
    rtol, atol = bar(kind, ref)
    torch.testing.assert_close(got.detach().cpu().double(), ref, rtol=rtol, atol=atol,
                               msg=lambda m: f"{what or kind}: {m}")


def _leaf(t: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """`t` itself when it already belongs to a graph in `dtype` (a composition), else a fresh leaf."""
    if t.dtype == dtype and t.requires_grad and t.device.type == "cpu":
        if not t.is_leaf:
            t.retain_grad()
        return t
    return t.detach().cpu().to(dtype).requires_grad_(True)


def encoder_params(seed: int = 11):
    """The nine encoder parameters (float32, CPU, ENCODER_PARAM_NAMES order) of a freshly seeded reference model."""
    torch.manual_seed(seed)
    ref = ref_model.RefGraphMETNetwork(8, 3, output_dim=1, hidden_dim=32, conv_depth=1)
    sd = dict(ref.named_parameters())
    return [sd[n].detach().float().clone() for n in ENCODER_PARAM_NAMES]


def encoder_inputs(N: int, seed: int):
    """(x_cont [N,8] float32, x_cat [N,3] int64 = pdgId, charge, fromPV, g_h [N,32] float32), unknown pdg ids included."""
    g = torch.Generator().manual_seed(seed)
    x_cont = torch.randn(N, 8, generator=g) * 2.0
    pdg_pool = torch.tensor(PDG_POOL)
    x_cat = torch.stack([pdg_pool[torch.randint(0, len(pdg_pool), (N,), generator=g)],
                         torch.randint(-1, 2, (N,), generator=g), torch.randint(0, 8, (N,), generator=g)], dim=1)
    g_h = torch.randn(N, 32, generator=g)
    return x_cont, x_cat, g_h


def encoder_ref(x_cont, x_cat, params, g_h=None, dtype=torch.float64):
    """(h [N,32] float64, leaves): the chain of graph_met_network.py:48-58 before bn_all, layer by layer in float64 --
    the sequential pdg remap (unknown ids keep their own value as the class), the three embeddings, the two input
    layers and encode_all.  `leaves` are the nine parameters as float64 leaves; with `g_h` given, h.backward(g_h) has run."""
    leaves = [_leaf(p, dtype) for p in params]
    Wc, bc, Wk, bk, Wa, ba, Echg, Epdg, Epv = leaves
    x_cat = x_cat.detach().cpu().long()
    pdg = x_cat[:, 0].abs()
    for cls, val in enumerate(ref_model._PDG_TABLE):
        pdg = torch.where(pdg == val, torch.full_like(pdg, cls), pdg)
    cat = torch.cat([F.embedding(x_cat[:, 1] + 1, Echg), F.embedding(pdg, Epdg), F.embedding(x_cat[:, 2], Epv)], dim=1)
    joint = torch.cat([F.elu(F.linear(cat, Wk, bk)), F.elu(F.linear(x_cont.detach().cpu().to(dtype), Wc, bc))], dim=1)
    h = F.elu(F.linear(joint, Wa, ba))
    if g_h is not None:
        h.backward(g_h.detach().cpu().to(dtype))
    return h, leaves


def head_params(seed: int = 3):
    """(W1 [16,32], b1 [16], W2 [1,16], b2 [1]) float32, CPU."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(16, 32, generator=g) * 0.3, torch.randn(16, generator=g) * 0.3,
            torch.randn(1, 16, generator=g) * 0.5, torch.randn(1, generator=g)]


def head_inputs(N: int, seed: int):
    """(emb [N,32], g_out [N]) float32, CPU."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 32, generator=g), torch.randn(N, generator=g)


def head_ref(emb, W1, b1, W2, b2, g_out=None, dtype=torch.float64):
    """(out [N] float64, leaves): sigmoid(Linear(ELU(Linear(emb)))); leaves = (emb, W1, b1, W2, b2) in float64.  `emb`
    may belong to a float64 graph already (bn_ref's output): its gradient is retained."""
    leaves = [_leaf(t, dtype) for t in (emb, W1, b1, W2, b2)]
    out = torch.sigmoid(F.linear(F.elu(F.linear(leaves[0], leaves[1], leaves[2])), leaves[3], leaves[4])).squeeze(-1)
    if g_out is not None:
        out.backward(g_out.detach().cpu().to(dtype))
    return out, leaves


def bn_state(H: int, seed: int):
    """A non-trivial BatchNorm1d(H) state (float32, CPU): weight in [0.5, 1.5), bias, running_mean, running_var in
    [0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    return {"weight": torch.rand(H, generator=g) + 0.5, "bias": torch.randn(H, generator=g),
            "running_mean": torch.randn(H, generator=g), "running_var": torch.rand(H, generator=g) + 0.5,
            "num_batches_tracked": torch.tensor(0)}


def bn_rows(N: int, H: int, seed: int):
    """(x [N,H], residual [N,H], g_y [N,H]) float32, CPU: x = 0.7 randn + 3 (a common offset, for the shifted sums); a
    handful of rows (N < 8) are spread instead, row i = row 0 + i * step with |step| in [0.5, 1.5) per channel, so that
    the batch variance is at least 1/16 in every channel (see "Inputs" in the module docstring)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, generator=g) * 0.7 + 3.0
    r = torch.randn(N, H, generator=g)
    g_y = torch.randn(N, H, generator=g)
    if N < 8:
        step = (torch.rand(H, generator=g) + 0.5) * (torch.randint(0, 2, (H,), generator=g) * 2 - 1)
        x = x[:1] + torch.arange(N, dtype=torch.float32)[:, None] * step
    return x, r, g_y


def bn_module(state, training: bool = True, dtype=torch.float32) -> torch.nn.BatchNorm1d:
    """torch.nn.BatchNorm1d with `state` loaded, in the given dtype and mode."""
    bn = torch.nn.BatchNorm1d(state["weight"].numel()).to(dtype)
    bn.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()})
    return bn.train(training)


def bn_ref(x, state, training: bool = True, residual=None, g_y=None, dtype=torch.float64):
    """(y float64, module, x leaf, residual leaf or None): torch.nn.BatchNorm1d(H).double() with `state` on x
    (+ residual).  `x` may be a float64 tensor that already belongs to a graph (encode_bn_ref): it is used as it is and
    returned in place of the leaf.  With `g_y` given, y.backward(g_y) has run; the module then holds the parameter
    gradients, the updated running statistics and num_batches_tracked."""
    ref = bn_module(state, training, dtype)
    x64 = _leaf(x, dtype)
    r64 = _leaf(residual, dtype) if residual is not None else None
    y = ref(x64)
    if r64 is not None:
        y = y + r64
    if g_y is not None:
        y.backward(g_y.detach().cpu().to(dtype))
    return y, ref, x64, r64


def encode_bn_ref(x_cont, x_cat, params, state, g_y=None, dtype=torch.float64):
    """(y float64, encoder leaves, module): training-mode bn_ref on encoder_ref's output, one graph."""
    h, leaves = encoder_ref(x_cont, x_cat, params, None, dtype)
    y, ref, _, _ = bn_ref(h, state, True, None, g_y, dtype)
    return y, leaves, ref


def bn_head_ref(raw, state, training, residual, head_params_, g_out=None, dtype=torch.float64):
    """(out, emb, module, raw leaf, residual leaf, head leaves): head_ref on bn_ref's output, one graph; head leaves[0] is
    emb with its gradient retained."""
    emb, ref, x64, r64 = bn_ref(raw, state, training, residual, None, dtype)
    out, leaves = head_ref(emb, *head_params_, g_out, dtype)
    return out, emb, ref, x64, r64, leaves
